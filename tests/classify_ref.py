"""The yardstick of the classification tests: the "Classification" section of include/geglove.h in numpy, operation for
operation.  Never the library itself.

numpy's fp64 `*`, `+`, `-`, `/` are single IEEE operations rounded to nearest even and never fused, so `p * r + c` below is the
header's unfused pair.  Sums whose order the header fixes go through kmeans_ref.seq_sum or a scalar loop; the two fmaf chains
(logits over ascending d, piece gradients over ascending members) are chain_ref.chain, which also asserts that no nonzero
product is below 2^-100: the header's 2^-60 cut on the probabilities together with features of magnitude >= 2^-20 keeps the
gradient's products at 2^-80 or more."""
import math

import numpy as np

import chain_ref as CH
import kmeans_ref as KM
import nn_ref
from geglove import synth

F32, F64 = np.float32, np.float64
PIECE = 1024
HISTORY, TRIALS = 8, 30
COSINE, RAW = "cosine", "none"
LN2HI, LN2LO, INVLN2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.4426950408889634
SQRT_HALF = 0.70710678118654752440
CUT = 2.0 ** -60
GRADIENT, MAXITER, LINESEARCH = "gradient", "maxiter", "linesearch"


def cexp(t):
    """cexp of the header on an array of t <= 0."""
    t = np.asarray(t, F64)
    assert np.all(t <= 0)
    small = t < -708.0
    tt = np.where(small, 0.0, t)
    k = np.rint(tt * INVLN2)
    r = (tt - k * LN2HI) - k * LN2LO
    p = np.full(tt.shape, 1.0 / float(math.factorial(13)))
    for j in range(12, -1, -1):
        p = p * r + 1.0 / float(math.factorial(j))
    return np.where(small, 0.0, np.ldexp(p, k.astype(np.int64)))


def clog(S):
    """clog of the header on an array of S >= 1."""
    S = np.asarray(S, F64)
    assert np.all(S >= 1)
    f, k = np.frexp(S)
    low = f < SQRT_HALF
    f = np.where(low, 2.0 * f, f)
    k = np.where(low, k - 1, k).astype(F64)
    s = (f - 1.0) / (f + 1.0)
    w = s * s
    q = np.full(S.shape, 1.0 / 25.0)
    for j in range(23, 0, -2):
        q = q * w + 1.0 / float(j)
    return k * LN2HI + (k * LN2LO + (2.0 * s) * q)


def features(X, normalize):
    """The prepared rows fp32 [n][dim + 1]: kmeans_ref.prepare, then the column of ones."""
    XH = KM.prepare(X, KM.COSINE if normalize == COSINE else KM.EUCLID)
    return np.concatenate([XH, np.ones((XH.shape[0], 1), F32)], axis=1)


def members(labels, train=None):
    labels = np.asarray(labels)
    live = labels >= 0
    if train is not None:
        live &= np.asarray(train) != 0
    return np.flatnonzero(live)


def logits(XH, W):
    """z fp32 [rows][C]: the fmaf chain over ascending d (the bias its last live product); non-finite values come back as they are."""
    return CH.chain(XH, np.asarray(W, F32))


def softmax(Z):
    """(T, E, S, PF) of finite fp32 logits [m][C]."""
    Z = np.asarray(Z, F32)
    rows = np.arange(Z.shape[0])
    m = Z[rows, np.argmax(Z, axis=1)]                        # fp32 compares, the first of equals
    T = Z.astype(F64) - m.astype(F64)[:, None]
    E = cexp(T)
    S = KM.seq_sum(E, 1)
    Q = E / S[:, None]
    PF = np.where(Q < CUT, F32(0), Q.astype(F32)).astype(F32)
    return T, E, S, PF


def residuals(Z, y):
    """(l fp64 [m], R fp32 [m][C])"""
    T, E, S, PF = softmax(Z)
    rows = np.arange(Z.shape[0])
    one = np.zeros(PF.shape, F32)
    one[rows, y] = 1
    return clog(S) - T[rows, y], (PF - one).astype(F32)


def partition_sum(v):
    return KM.partition_sum(v)


def scalar_sum(values):
    s = 0.0
    for v in np.asarray(values, F64).ravel().tolist():
        s = s + v
    return s


def dot(a, b):
    return scalar_sum(np.asarray(a, F64) * np.asarray(b, F64))


def piece_gradients(R, XT):
    """Gp fp32 [pieces][C][Dp]: per piece the fmaf chain over its members in ascending t."""
    return np.stack([CH.chain(R[i:i + PIECE].T, XT[i:i + PIECE].T) for i in range(0, R.shape[0], PIECE)])


def evaluate(XH, labels, train, W, l2):
    """(f, g fp64 [C][Dp]) at the fp32 weights W [C][Dp], or None when a logit of a member is not finite."""
    W = np.ascontiguousarray(W, F32)
    mem = members(labels, train)
    y = np.asarray(labels)[mem]
    XT = XH[mem]
    dim = XH.shape[1] - 1
    Z = logits(XT, W)
    if not np.all(np.isfinite(Z)):
        return None
    l, R = residuals(Z, y)
    n_t = float(len(mem))
    W64 = W.astype(F64)
    reg = scalar_sum(W64[:, :dim] * W64[:, :dim])
    f = partition_sum(l) / n_t + (0.5 * l2) * reg
    G = KM.seq_sum(piece_gradients(R, XT).astype(F64), 0)
    g = G / n_t
    g[:, :dim] = g[:, :dim] + l2 * W64[:, :dim]
    return float(f), g


def plain_gradient(XH, labels, train, W, l2):
    """The textbook softmax gradient in fp64 with numpy's own exp and matrix product, and sum_t sum|r||x| / n_T per element."""
    mem = members(labels, train)
    y = np.asarray(labels)[mem]
    X64, W64 = XH[mem].astype(F64), np.asarray(W, F32).astype(F64)
    dim = XH.shape[1] - 1
    Z = X64 @ W64.T
    Z -= Z.max(axis=1, keepdims=True)
    P = np.exp(Z)
    P /= P.sum(axis=1, keepdims=True)
    P[np.arange(len(mem)), y] -= 1.0
    g = P.T @ X64 / len(mem)
    g[:, :dim] += l2 * W64[:, :dim]
    return g, np.abs(P).T @ np.abs(X64) / len(mem)


class Fit:
    """The optimiser of the header: state theta, f, g, the history (oldest first), it; run(max_iter) as ge_classify_run."""

    def __init__(self, XH, labels, train, classes, l2=1e-4, tolerance=1e-4, weights=None):
        self.XH, self.labels, self.train, self.C, self.l2, self.tol = XH, np.asarray(labels), train, classes, l2, tolerance
        self.Dp = XH.shape[1]
        self.theta = np.zeros(classes * self.Dp, F64) if weights is None else np.asarray(weights, F32).astype(F64).ravel()
        self.H, self.have, self.f, self.g = [], False, 0.0, None
        self.iterations, self.evaluations, self.stop = 0, 0, "none"
        self.losses = []

    def weights(self, theta=None):
        return (self.theta if theta is None else theta).astype(F32).reshape(self.C, self.Dp)

    def eval_at(self, theta):
        out = evaluate(self.XH, self.labels, self.train, self.weights(theta), self.l2)
        return None if out is None else (out[0], out[1].ravel())

    def run(self, max_iter):
        assert max_iter >= 1
        if not self.have:
            out = self.eval_at(self.theta)
            assert out is not None, "non-finite logit"
            self.evaluations += 1
            self.f, self.g = out
            self.have = True
            self.losses.append(self.f)
        ran = 0
        while True:
            if np.abs(self.g).max() <= self.tol:
                self.stop = GRADIENT
                break
            if ran >= max_iter:
                self.stop = MAXITER
                break
            q = self.g.copy()
            a = [0.0] * len(self.H)
            for j in range(len(self.H) - 1, -1, -1):
                s, y, sy = self.H[j]
                a[j] = dot(s, q) / sy
                q = q - a[j] * y
            if self.H:
                s, y, sy = self.H[-1]
                q = (sy / dot(y, y)) * q
            for j in range(len(self.H)):
                s, y, sy = self.H[j]
                b = dot(y, q) / sy
                q = q + (a[j] - b) * s
            d = -q
            dg = dot(d, self.g)
            if not dg < 0:
                self.H = []
                d = -self.g
                dg = dot(d, self.g)
            alpha = 1.0 if self.H else 1.0 / max(1.0, math.sqrt(dot(self.g, self.g)))
            accepted = None
            for _ in range(TRIALS):
                trial = self.theta + alpha * d
                out = self.eval_at(trial)
                self.evaluations += 1
                if out is not None and out[0] <= self.f + (1e-4 * alpha) * dg:
                    accepted = out
                    break
                alpha = 0.5 * alpha
            if accepted is None:
                if self.H:
                    self.H = []
                    continue
                self.stop = LINESEARCH
                break
            s, y = trial - self.theta, accepted[1] - self.g
            sy = dot(s, y)
            if sy > 1e-10 * dot(y, y):
                self.H.append((s, y, sy))
                self.H = self.H[-HISTORY:]
            self.theta, self.f, self.g = trial, accepted[0], accepted[1]
            self.iterations += 1
            ran += 1
            self.losses.append(self.f)
        return ran, self.stop


def predict(XH, W):
    """(label int32 [n], prob fp32 [n]) of every position, or None when a logit is not finite."""
    Z = logits(XH, W)
    if not np.all(np.isfinite(Z)):
        return None
    label, _ = KM.assign(Z)                                  # the total order of ge_nn_*
    T, E, S, PF = softmax(Z)
    return label.astype(np.int32), (1.0 / S).astype(F32)


def score(labels, predicted, mask, classes):
    """dict as capi.Classifier.score, from a numpy confusion matrix."""
    labels, predicted = np.asarray(labels), np.asarray(predicted)
    take = labels >= 0
    if mask is not None:
        take &= np.asarray(mask) != 0
    conf = np.zeros((classes, classes), np.int64)
    np.add.at(conf, (labels[take], predicted[take]), 1)
    tp = np.diag(conf).copy()
    fp, fn = conf.sum(axis=0) - tp, conf.sum(axis=1) - tp
    count, correct = int(conf.sum()), int(tp.sum())
    f1 = [2.0 * float(tp[c]) / float(2 * tp[c] + fp[c] + fn[c]) for c in range(classes) if tp[c] + fp[c] + fn[c] > 0]
    return {"count": count, "correct": correct, "accuracy": correct / count if count else 0.0,
            "macro_f1": scalar_sum(f1) / float(len(f1)) if f1 else 0.0, "tp": tp, "fp": fp, "fn": fn, "confusion": conf}


# ---- inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------

def planted(seed, n, dim, classes, noise=0.25):
    """`classes` centres on the unit sphere; position p belongs to class (p + p // classes) mod classes (every class on both sides of a
    split that takes every k-th position) and lies at centre + noise * uniform / sqrt(dim), pushed through a fixed ill-conditioned diagonal-plus-shear mix."""
    Cn = nn_ref.uniform(seed, (classes, dim))
    Cn /= np.linalg.norm(Cn, axis=1, keepdims=True)
    p = np.arange(n)
    y = ((p + p // classes) % classes).astype(np.int32)
    X = Cn[y] + noise / np.sqrt(dim) * nn_ref.uniform(seed + 1, (n, dim))
    M = np.diag(np.exp2(np.linspace(-2, 2, dim))) + 0.25 * np.eye(dim, k=1)
    return (X @ M).astype(F32), y


def features_in_range(XH):
    a = np.abs(XH[XH != 0]).astype(F64)
    return a.size == 0 or (a.min() >= 2.0 ** -20 and a.max() <= 2.0 ** 20)


def case_rows(seed, n, dim):
    """Rows whose components have magnitudes in [1/2, 2): prepared under either normalisation they stay inside [2^-20, 2^20]."""
    u = nn_ref.uniform(seed, (n, dim))
    return (np.sign(u + 1e-300) * (0.5 + 1.5 * np.abs(u))).astype(F32)


def case_weights(seed, classes, dp, scale=1.0):
    """Finite weights of magnitude in [scale / 16, scale]: no product of the logit chain is near the subnormal range."""
    u = nn_ref.uniform(seed, (classes, dp))
    return (scale * np.sign(u + 1e-300) * (1.0 / 16 + 15.0 / 16 * np.abs(u))).astype(F32)


# (name, n, n_T, dim, C, normalize, subset, a class without members): every C, dim and n_T the tile edges ask for appears once
CASES = [
    ("one-member", 9, 1, 1, 2, COSINE, False, False),
    ("c3-d3", 200, 63, 3, 3, RAW, False, False),
    ("c16-d4", 150, 64, 4, 16, COSINE, True, False),
    ("c17-d31", 130, 65, 31, 17, RAW, False, True),
    ("c128-d32", 1500, 1023, 32, 128, COSINE, False, False),
    ("c129-d33", 1300, 1024, 33, 129, RAW, True, False),
    ("c200-d3", 1400, 1025, 3, 200, COSINE, False, True),
    ("c2-d200", 3000, 2500, 200, 2, COSINE, False, False),
    ("c5-d200-raw", 300, 200, 200, 5, RAW, False, False),
]
EDGES = {"C": {2, 3, 16, 17, 128, 129, 200}, "dim": {1, 3, 4, 31, 32, 33, 200}, "n_T": {1, 63, 64, 65, 1023, 1024, 1025, 2500}}


def build_case(case):
    """dict: rows (the table handed to create), subset, X (the indexed rows), labels, train, W, XH, classes, normalize.  Unlabelled
    and labelled-but-not-training positions are interleaved with the members; `empty` leaves class 1 without a member."""
    name, n, n_t, dim, classes, normalize, subset, empty = case
    seed = 1000 + 17 * len(name) + dim + classes
    n_rows = n + 7 if subset else n
    rows = case_rows(seed, n_rows, dim)
    sub = None
    if subset:
        drop = np.argsort(synth.splitmix64(seed + 1, n_rows), kind="stable")[:7]
        sub = np.setdiff1d(np.arange(n_rows), drop).astype(np.int32)
    X = rows[sub] if subset else rows
    order = np.argsort(synth.splitmix64(seed + 2, n), kind="stable")
    mem = np.sort(order[:n_t])
    rest = order[n_t:]
    labels = np.full(n, -1, np.int32)
    train = np.zeros(n, np.uint8)
    ids = (synth.splitmix64(seed + 3, n) % np.uint64(classes)).astype(np.int32)
    if empty:
        ids[ids == 1] = 0
    labels[mem] = ids[mem]
    train[mem] = 1
    held = rest[::2]                                         # labelled, not training
    labels[held] = ids[held]
    train[rest[1::4]] = 1                                    # a train flag on an unlabelled position means nothing
    if n_t == n:
        train = None
    W = case_weights(seed + 4, classes, dim + 1)
    XH = features(X, normalize)
    return {"name": name, "rows": rows, "subset": sub, "X": X, "labels": labels, "train": train, "W": W, "XH": XH, "classes": classes,
            "normalize": normalize, "dim": dim, "n_t": n_t, "empty": empty}


def under_the_cut_case():
    """Two members whose logits differ by more than 60 ln 2 ~ 41.6: the loser's probability falls under the 2^-60 cut and its
    residual is exactly 0.0f (or -1.0f for the true class)."""
    X = np.array([[1, 0], [0, 1], [1, 1], [-1, 0]], F32)
    labels = np.array([0, 1, 1, 0], np.int32)
    W = np.array([[50, -50, 0.5], [-50, 50, -0.5], [1, 1, 0.25]], F32)
    return {"name": "cut", "rows": X, "subset": None, "X": X, "labels": labels, "train": None, "W": W, "XH": features(X, RAW), "classes": 3,
            "normalize": RAW, "dim": 2, "n_t": 4, "empty": False}

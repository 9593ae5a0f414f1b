"""Designed co-occurrence matrices for the trainer tests (test_designed_matrices.py, test_designed_matrices_gpu.py).

geglove.synth gives hub-heavy random matrices: X in (1e-4, 0.2] with xmax the largest X, unique (i, j), a diagonal entry per row.
The generators here build the inputs that family never produces, one structure at a time, so that a test with a known right
answer walks them:
  * one_column / one_row   one hub run of n nonzeros (cut by chunk and by flush limit), or a new resident row at every step
                           with the SAME streamed row behind the previous step's stores;
  * repeats                the same (i, j) several times back to back, and again later;
  * alternating            one resident row whose streamed side alternates between two rows (and the transpose);
  * partial(n)             conflict-free batches that do not fill their last chunk;
  * glove_edge_x / pglove_edge_x   X on and around xmax (xmax a double fp32 cannot hold), far above it, subnormal, huge,
                           pGloVe's X -> 1 and X = 0.5.
Everything is plain numpy seeded through synth.splitmix64; each generator returns (V, I, J, X, xmax).

Structure matrices draw X log-uniformly from [0.02, 0.2] with xmax 0.2: the weight (X / xmax)^0.75 is then at least 0.18 and
|log X| at least 1.6, so every single update moves the tables by far more than a replay tolerance and none can be lost or applied
to a stale row unseen (test_designed_matrices.py checks that condition nonzero by nonzero).
Test infrastructure only."""
import numpy as np

from geglove import synth

F32 = np.float32
XMAX = float(F32(0.2))            # what synth.synthetic_coo passes as xmax: the largest X, widened


def _u01(seed, n, offset=0):
    return (synth.splitmix64(seed, n, offset) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _ints(seed, n, bound):
    return np.minimum((_u01(seed, n) * bound).astype(np.int64), bound - 1)


def structure_x(seed, n):
    """n values log-uniform in [0.02, 0.2], fp32."""
    x = np.exp(np.log(0.02) + _u01(seed ^ 0x0F0F0F0F, n) * np.log(10.0))
    return np.clip(x, 0.02, 0.2).astype(F32)


def _pack(V, I, J, X, xmax):
    return int(V), np.asarray(I, np.int32), np.asarray(J, np.int32), np.asarray(X, F32), float(xmax)


def one_column(n=300, seed=101):
    """Rows 0..n-1 with one nonzero each, all in column n."""
    return _pack(n + 1, np.arange(n), np.full(n, n), structure_x(seed, n), XMAX)


def one_row(n=300, seed=102):
    """The transpose: row n with one nonzero in each of the columns 0..n-1."""
    return _pack(n + 1, np.full(n, n), np.arange(n), structure_x(seed, n), XMAX)


REPEAT_ROWS, REPEAT_COLS, REPEAT_DRAWS = 7, 11, 40


def repeats(seed=182):
    """40 draws of a pair (i, j) from 7 rows x 11 columns, each written 1..5 times back to back (every copy with an X of its own).
    The draws are with replacement, so some pairs come back later in the array.
    The biases take AdaGrad steps without a learning rate, so on so few rows a residual can pass close to zero, and an update with
    a residual near zero moves nothing: the default seed is one whose every nonzero is visible at every dim the tests use (of the
    seeds 123..400 one in sixteen is; test_designed_matrices.py holds this one to the condition)."""
    i = _ints(seed, REPEAT_DRAWS, REPEAT_ROWS)
    j = _ints(seed ^ 0x5A5A5A5A, REPEAT_DRAWS, REPEAT_COLS)
    times = 1 + _ints(seed ^ 0x77777777, REPEAT_DRAWS, 5)
    I = np.repeat(i, times); J = np.repeat(j, times)
    return _pack(max(REPEAT_ROWS, REPEAT_COLS), I, J, structure_x(seed, len(I)), XMAX)


def alternating(seed=351, n=40):
    """Row 0 alternating between columns 1 and 2 (n nonzeros), then column 3 alternating between rows 4 and 5 (n nonzeros).
    (The default seed is chosen like that of repeats(): six rows fit their residuals fast.)"""
    k = np.arange(n)
    I = np.concatenate([np.zeros(n, np.int64), 4 + (k & 1)])
    J = np.concatenate([1 + (k & 1), np.full(n, 3)])
    return _pack(6, I, J, structure_x(seed, 2 * n), XMAX)


STRUCTURES = {"one_column": one_column, "one_row": one_row, "repeats": repeats, "alternating": alternating}

PARTIAL_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 193)


def partial(n, spare=37):
    """synth.conflict_free_batch with n nonzeros (all i distinct, all j distinct) in a vocabulary of n + spare: the last chunk of
    128 holds n % 128 nonzeros, and `spare` rows on either side are touched by nothing."""
    V = n + spare
    I, J, X = synth.conflict_free_batch(V, n, seed=1000 + n)
    return _pack(V, I, J, X, XMAX)


def _conflict_free(V, n, seed):
    pi = np.argsort(synth.splitmix64(seed, V), kind="stable")[:n]
    pj = np.argsort(synth.splitmix64(seed ^ 0xABCDEF, V), kind="stable")[:n]
    return pi, pj


GLOVE_EDGE_XMAX = 0.3             # a double fp32 cannot hold: fp32(0.3) = 0.300000011920929 > 0.3


def glove_edge_values():
    x3 = F32(0.3)
    return np.array([x3, np.nextafter(x3, F32(0)), np.nextafter(x3, F32(1)), 0.6, 300.0, 1.0, 1e-30,
                     np.finfo(F32).tiny, 1e-40], F32)


def glove_edge_x(seed=105, spare=9):
    """Conflict-free, one nonzero per value of glove_edge_values(), xmax = 0.3 as a double.  fp32(0.3) exceeds it (weight 1), its
    lower neighbour does not (weight just under 1): an fp32 comparison, or an xmax narrowed to fp32, gets one of the two wrong."""
    X = glove_edge_values()
    V = len(X) + spare
    I, J = _conflict_free(V, len(X), seed)
    return _pack(V, I, J, X, GLOVE_EDGE_XMAX)


def pglove_edge_values():
    return np.array([0.5, 1.0 - 2.0 ** -24, 0.999, 2.0 ** -24, 1e-30, 1e-40], F32)


def pglove_edge_x(seed=106, spare=9):
    """Conflict-free, one nonzero per value of pglove_edge_values(): l = log(X / (1 - X)) is 0 at 0.5 and log(2^24 - 1) at the
    largest fp32 below 1.  (xmax plays no part in pGloVe's cost; the largest X is passed, as BookmarkColoring would.)"""
    X = pglove_edge_values()
    V = len(X) + spare
    I, J = _conflict_free(V, len(X), seed)
    return _pack(V, I, J, X, float(X.max()))


def hub_column(rows=3000, seed=107):
    """`rows` rows with one nonzero each in one shared column (id `rows`): one_column at a size where many workers meet."""
    return one_column(rows, seed)


# ---------------------------------------------------------------------------------------------------------------------------
# structure facts the CPU test asserts and the GPU tests rely on
def back_to_back(I, J):
    """Lengths of the maximal groups of consecutive equal (i, j)."""
    I = np.asarray(I); J = np.asarray(J)
    cut = np.nonzero((I[1:] != I[:-1]) | (J[1:] != J[:-1]))[0] + 1
    return np.diff(np.concatenate([[0], cut, [len(I)]]))


def is_conflict_free(I, J):
    return len(np.unique(I)) == len(I) and len(np.unique(J)) == len(J)


def replay_tolerance(ref_table):
    """Per-element tolerance of the one-worker replays (helpers.assert_state_equal with rtol 5e-5, atol 5e-6 of the table's largest
    magnitude)."""
    b = np.asarray(ref_table, np.float64)
    return 5e-5 * np.abs(b) + 5e-6 * (float(np.max(np.abs(b))) if b.size else 1.0)


def tolerance_share(got, ref, rtol, atol):
    """Largest |got - ref| / (rtol |ref| + atol max|ref|) over the tables of two state dicts: the share of an
    assert_state_equal(exact=False) tolerance that is used (> 1 fails)."""
    worst, where = 0.0, ""
    for name in got:
        a = np.asarray(got[name], np.float64).reshape(-1); b = np.asarray(ref[name], np.float64).reshape(-1)
        tol = rtol * np.abs(b) + atol * (float(np.max(np.abs(b))) if b.size else 1.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.where(a == b, 0.0, np.abs(a - b) / tol)
        s = np.where(np.isnan(s), np.inf, s)
        if s.size and float(s.max()) > worst:
            worst, where = float(s.max()), "%s[%d]" % (name, int(np.argmax(s)))
    return worst, where

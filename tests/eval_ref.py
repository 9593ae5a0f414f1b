"""The held-out evaluation of include/geglove.h restated in numpy, and the oracle it is held to.

model(state, D, I, J, X, xmax, cost) -> (residual float32[n], term float64[n]): float32 products, a sequential float32 sum in
ascending d from 0.0f, fp64 for the rest -- the arithmetic of exact_update (csrc/ge_exact.h) stopped before the update.  log and
pow go through libm one value at a time (math.log / math.pow), as the oracle's C does.
partitioned_sum(term) -> cost_sum: S_b over [1024 b, 1024 (b + 1)) in ascending k, then the S_b in ascending b, all from 0.0.
oracle_terms(...) -> float32[n]: (float)t_k from the oracle itself, one one-nonzero job per k on a copy of the state
(oracle.adagrad_job, or oracle.opt_job for Adam / AMSGrad states).
holdout_mask(seed, n, fraction): the split rule, SplitMix64 in numpy.
"""
import math

import numpy as np

import oracle as O
from geglove import synth

SUM_BLOCK = 1024
HOLDOUT_SALT = 0x484F4C444F5554
F32 = np.float32


def _lw(x, xmax, cost):
    """cost_terms<true> (csrc/ge_cost.h): (l as a python float, w as float32) of one value"""
    x = F32(x)
    if cost == O.COST_GLOVE:
        l = math.log(float(x))
        w = F32(1.0) if float(x) > xmax else F32(math.pow(float(x) / xmax, 0.75))
    else:
        l = math.log(float(F32(x / (F32(1.0) - x))))
        w = x
    return l, w


def model(state, D, I, J, X, xmax, cost, row_begin=0):
    """state: the tables as ge_glove_get_state returns them (focus-side tables hold the rows from row_begin on)."""
    I = np.asarray(I, np.int64); J = np.asarray(J, np.int64); X = np.ascontiguousarray(X, F32)
    focus = np.asarray(state["focus"], F32).reshape(-1, D); context = np.asarray(state["context"], F32).reshape(-1, D)
    fbias = np.asarray(state["fbias"], F32).reshape(-1); cbias = np.asarray(state["cbias"], F32).reshape(-1)
    prod = focus[I - row_begin] * context[J]                      # float32 x float32: rounded once, never fused
    assert prod.dtype == F32
    s = np.zeros(len(I), F32)
    for d in range(D):
        s = s + prod[:, d]                                        # ascending d, float32
    assert s.dtype == F32
    lw = [_lw(x, xmax, cost) for x in X]
    l = np.array([a for a, _ in lw], np.float64); w = np.array([b for _, b in lw], F32)
    bias = (fbias[I - row_begin] + cbias[J]).astype(F32)
    ic = (s.astype(np.float64) + (bias.astype(np.float64) - l)).astype(F32)
    wc = w * ic
    assert wc.dtype == F32
    term = (0.5 * wc.astype(np.float64)) * ic.astype(np.float64)
    return ic, term


def partitioned_sum(term):
    total = 0.0
    for b0 in range(0, len(term), SUM_BLOCK):
        sb = 0.0
        for t in term[b0:b0 + SUM_BLOCK].tolist():
            sb = sb + t
        total = total + sb
    return total


_TOUCHED = (("focus", 0), ("context", 1), ("fbias", 0), ("cbias", 1), ("gsq_focus", 0), ("gsq_context", 1), ("gsq_fbias", 0),
            ("gsq_cbias", 1), ("m2_focus", 0), ("m2_context", 1), ("m2_fbias", 0), ("m2_cbias", 1))


def oracle_terms(state, V, D, I, J, X, xmax, cost, opt=O.OPT_ADAGRAD, iteration=0, row_begin=0):
    """(float)t_k of every nonzero from one-nonzero oracle jobs.  The job runs on a working copy of the state whose touched rows are
    put back from the pristine copy afterwards -- the same as a fresh copy per job.  A shard's focus-side tables are placed at
    their global rows first (the oracle indexes by global row id)."""
    names = [n for n, _ in _TOUCHED if n in state]
    if opt != O.OPT_ADAGRAD:
        assert len(names) == 12
    pristine = {}
    for name, side in _TOUCHED:
        if name not in state:
            continue
        width = D if name.endswith(("focus", "context")) else 1
        a = np.asarray(state[name], F32).reshape(-1, width)
        if side == 0 and a.shape[0] != V:
            full = np.ones((V, width), F32)
            full[row_begin:row_begin + a.shape[0]] = a
            a = full
        pristine[name] = np.ascontiguousarray(a)
    work = {k: v.copy() for k, v in pristine.items()}
    flat = {k: v.reshape(-1) if v.shape[1] == 1 else v for k, v in work.items()}
    out = np.empty(len(I), F32)
    for k in range(len(I)):
        i, j = int(I[k]), int(J[k])
        if opt == O.OPT_ADAGRAD:
            out[k] = O.adagrad_job(D, [i], [j], [X[k]], xmax, cost, flat)
        else:
            out[k] = O.opt_job(opt, iteration, D, [i], [j], [X[k]], xmax, cost, flat)
        for name, side in _TOUCHED:
            if name in work:
                r = i if side == 0 else j
                work[name][r] = pristine[name][r]
    return out


def holdout_mask(seed, n, fraction):
    T = int(math.floor(float(fraction) * 4294967296.0))
    u = synth.splitmix64((seed ^ HOLDOUT_SALT) & 0xFFFFFFFFFFFFFFFF, n, 0)
    return ((u >> np.uint64(32)) < np.uint64(T)).astype(np.uint8)


def bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)

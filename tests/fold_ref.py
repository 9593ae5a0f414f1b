"""The fold-in section of include/geglove.h restated in numpy from the header alone: a new row fitted against frozen rows by the
AdaGrad update of GE_ARITH_FP32 with the other side left alone, word for word.  The dot product and the reduction tree are
kernel_model's (fma32, lane_dot, lane_shape), the cost terms strata_fp32_ref's, the keyed walk strata_ref's (keys, bijection).
Test infrastructure only."""
import numpy as np

import kernel_model as KM
import strata_fp32_ref as SF
import strata_ref as SR

F32, F64 = np.float32, np.float64
SHUFFLE_NONE, SHUFFLE_DEVICE = "none", "device"


def fold_row(D, ids, x, table, bias, xmax, pglove, epochs, shuffle, seed, lr, init_row=None, init_bias=0.0, base=0):
    """One new row: ids / x its nonzeros in the caller's order, table[id - base] / bias[id - base] the frozen side (fp32 arrays
    holding the values the device reads: bf16 rows widened, master rows where the handle keeps them).
    Returns (a float32[D], fb float32, c float32[epochs])."""
    vw, nch, _ = KM.lane_shape(D)
    lr = F32(lr)
    ids = np.asarray(ids, np.int64)
    x = np.asarray(x, F32)
    n = len(ids)
    a = np.zeros(D, F32) if init_row is None else np.array(init_row, F32)
    fb = F32(init_bias)
    Ga, Gfb = np.ones(D, F32), F32(1)
    terms = [SF.cost_terms(pglove, v, xmax) for v in x]
    c = np.zeros(epochs, F32)
    for e in range(epochs):
        walk = SR.bijection(n, SR.keys(seed, e, 0)) if shuffle == SHUFFLE_DEVICE else np.arange(n)
        ce = F32(0)
        for k in walk.tolist():
            l, w = terms[k]
            b = np.asarray(table[ids[k] - base], F32)
            dot = KM.lane_dot(a, b, vw, nch)
            ic = F32(F64(dot) + (F64(F32(fb + F32(bias[ids[k] - base]))) - l))
            wc = F32(w * ic)
            ce = F32(F64(ce) + (F64(0.5) * F64(wc)) * F64(ic))
            with np.errstate(all="ignore"):
                g = (wc * b).astype(F32)
                a = (a - ((g / np.sqrt(Ga)).astype(F32) * lr).astype(F32)).astype(F32)
                Ga = (Ga + (g * g).astype(F32)).astype(F32)
                fb = F32(fb - F32(wc / np.sqrt(Gfb)))
                Gfb = F32(Gfb + F32(wc * wc))
        c[e] = ce
    return a, fb, c


def fold(D, row_ptr, idx, X, table, bias, xmax, pglove=False, epochs=10, shuffle=SHUFFLE_DEVICE, seed=0, lr=0.05, init_rows=None,
         init_bias=None, base=0):
    """A whole set: (rows float32[n, D], bias float32[n], c float32[n, epochs], history float64[epochs]).  Rows are independent."""
    row_ptr = np.asarray(row_ptr, np.int64)
    n = len(row_ptr) - 1
    rows, fbs, c = np.zeros((n, D), F32), np.zeros(n, F32), np.zeros((n, epochs), F32)
    for r in range(n):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        rows[r], fbs[r], c[r] = fold_row(D, idx[lo:hi], X[lo:hi], table, bias, xmax, pglove, epochs, shuffle, seed, lr,
                                         None if init_rows is None else init_rows[r], 0.0 if init_bias is None else init_bias[r], base)
    history = np.zeros(epochs, F64)
    for e in range(epochs):
        total = 0.0
        for r in range(n):
            total = total + float(c[r, e])
        history[e] = total
    return rows, fbs, c, history


def frozen_side(state, side, D, vocab, rows=None):
    """(table, bias, base) of the side a fold-in reads, from the dict ge_glove_get_state fills: side "focus" reads the context rows
    and cBias of all `vocab` columns, side "context" the focus rows and fBias of the owned rows [rows[0], rows[1])."""
    if side == "focus":
        return state["context"].reshape(vocab, D), state["cbias"], 0
    n = rows[1] - rows[0] if rows else vocab
    return state["focus"].reshape(n, D), state["fbias"], rows[0] if rows else 0


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)

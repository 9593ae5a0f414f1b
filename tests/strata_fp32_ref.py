"""GE_ARITH_FP32 restated in numpy from include/geglove.h alone: the arithmetic of one update of a stratified handle whose
arithmetic is fp32, word for word.  The dot product, the reduction tree and the moment step are kernel_model's (fma32, lane_dot,
wave_sum, moment_step: what k_adagrad_runs already answers to); the order is strata_ref.Model's; what is new here is the AdaGrad
step in fp32, the exact mode's cost terms (libm pow) and the fp32 cost of a tile.  Test infrastructure only."""
import math

import numpy as np

import kernel_model as KM

F32, F64 = np.float32, np.float64
FOCUS_SIDE = ("focus", "fbias", "gsq_focus", "gsq_fbias", "m2_focus", "m2_fbias")


def cost_terms(pglove, x, xmax):
    """ge_cost.h cost_terms<true>: (l fp64, w fp32) of one nonzero, libm log and pow."""
    x = F32(x)
    if pglove:
        return F64(math.log(float(F32(x / F32(F32(1) - x))))), x
    w = F32(1) if float(x) > float(xmax) else F32(math.pow(float(x) / float(xmax), 0.75))
    return F64(math.log(float(x))), w


def tile(opt, iteration, D, I, J, X, xmax, state, pglove=False, lr=0.05):
    """The updates of one tile, in the given order, on the state dict (2-D row tables and 1-D bias tables, changed in place).
    opt: "adagrad" | "adam" | "amsgrad".  Returns the tile's fp32 cost."""
    vw, nch, _ = KM.lane_shape(D)
    lr = F32(lr)
    foc, ctx, fb, cb = state["focus"], state["context"], state["fbias"], state["cbias"]
    gf, gc, gfb, gcb = state["gsq_focus"], state["gsq_context"], state["gsq_fbias"], state["gsq_cbias"]
    mom = opt != "adagrad"
    if mom:
        ams = opt == "amsgrad"
        corr = lr if ams else KM.adam_correction(lr, iteration)
        hf, hc, hfb, hcb = state["m2_focus"], state["m2_context"], state["m2_fbias"], state["m2_cbias"]
    cost = F32(0)
    for i, j, x in zip(np.asarray(I).tolist(), np.asarray(J).tolist(), np.asarray(X, F32).tolist()):
        l, w = cost_terms(pglove, x, xmax)
        a, b = foc[i].copy(), ctx[j].copy()
        dot = KM.lane_dot(a, b, vw, nch)
        ic = F32(F64(dot) + (F64(F32(fb[i] + cb[j])) - l))
        wc = F32(w * ic)
        cost = F32(F64(cost) + (F64(0.5) * F64(wc)) * F64(ic))
        g1, g2 = (wc * b).astype(F32), (wc * a).astype(F32)
        if mom:
            st, gf[i], hf[i] = KM.moment_step(ams, corr, g1, gf[i], hf[i])
            foc[i] = (a - st).astype(F32)
            st, gc[j], hc[j] = KM.moment_step(ams, corr, g2, gc[j], hc[j])
            ctx[j] = (b - st).astype(F32)
            st, gfb[i], hfb[i] = KM.moment_step(ams, corr, wc, gfb[i], hfb[i]); fb[i] = F32(fb[i] - st)
            st, gcb[j], hcb[j] = KM.moment_step(ams, corr, wc, gcb[j], hcb[j]); cb[j] = F32(cb[j] - st)
        else:
            foc[i] = (a - ((g1 / np.sqrt(gf[i])).astype(F32) * lr).astype(F32)).astype(F32)
            ctx[j] = (b - ((g2 / np.sqrt(gc[j])).astype(F32) * lr).astype(F32)).astype(F32)
            gf[i] = (gf[i] + (g1 * g1).astype(F32)).astype(F32)
            gc[j] = (gc[j] + (g2 * g2).astype(F32)).astype(F32)
            fb[i] = F32(fb[i] - F32(wc / np.sqrt(gfb[i])))
            cb[j] = F32(cb[j] - F32(wc / np.sqrt(gcb[j])))
            gfb[i] = F32(gfb[i] + F32(wc * wc))
            gcb[j] = F32(gcb[j] + F32(wc * wc))
    return cost


def epoch(model, seed, iteration, shuffle, opt, D, I, J, X, xmax, state, pglove=False, lr=0.05):
    """One stratified epoch in its sequential order (strata_ref.Model.jobs), tile by tile.  Returns *cost_sum: the fp64 sum of the
    fp32 tile costs in epoch order."""
    total = 0.0
    for nz in model.jobs(seed, iteration, shuffle):
        if len(nz):
            total += float(tile(opt, iteration, D, I[nz], J[nz], X[nz], xmax, state, pglove, lr))
    return total

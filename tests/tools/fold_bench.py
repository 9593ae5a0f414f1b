"""The fold-in kernel at a serving shape.
    python tests/tools/fold_bench.py [--vocab 1000000] [--dim 200] [--rows 100000] [--nnz 10000000] [--epochs 10] [--reps 5]
                                     [--out profiles/fold_bench.json]

A HOGWILD handle of --vocab vertices and --dim columns is created on a ge_synth_coo matrix and trained for one epoch (the tables
need not be good, only in their trained places).  The new rows are the rows [0, --rows) of another ge_synth_coo matrix (another
seed) of --nnz nonzeros, folded in on the focus side for --epochs epochs under shuffle: device.  In this one process:
  * device time of ge_glove_fold_run (ge_fold_last_kernel_ms: hipEvents around the one launch): one warm-up run, then --reps
    runs; median, min, max;
  * updates per second; the bytes the updates must read -- a frozen row and 20 bytes of (idx, l, w, bias) each -- the rate that
    gives, and ge_copy_bandwidth measured here beside it;
  * `path` (ge_fold_get: epochs x the longest row) and the time of a set that holds the longest row alone, as a share of the
    whole set's time: what the one-wave-per-row rule costs on this input;
  * beside it the GE_ARITH_FP32 figures of profiles/strata_fp32_bench.json (dim 200), the existing yardstick of a wave-sequential
    update -- which loads two rows with their accumulators and stores them, where a fold-in loads one row and stores none.
No counters are taken and no threshold is set.  One JSON document on stdout, and in --out."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
import numpy as np                   # noqa: E402
import geglove                       # noqa: E402
from geglove import capi             # noqa: E402


def config(dim):
    return geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": dim, "threads": 1,
                                  "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                  "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                  "device": {"mode": "hogwild", "shuffle": "device", "seed": 42}})


def timed(fold, reps):
    fold.run()                                                            # warm-up
    ms = []
    for _ in range(reps):
        fold.run()
        ms.append(fold.kernel_ms)
    return ms


def yardstick():
    path = os.path.join(ROOT, "profiles", "strata_fp32_bench.json")
    if not os.path.exists(path):
        return None
    case = [c for c in json.load(open(path))["cases"] if c["dim"] == 200][0]
    best = [s for s in case["strata"] if s["strata"] == case["fastest_fp32_strata"]][0]
    return {"source": "profiles/strata_fp32_bench.json", "case": case["case"], "dim": case["dim"], "strata": best["strata"],
            "t_update_us": best["fp32"]["t_update_us"], "updates_per_s": best["fp32"]["updates_per_s"],
            "note": "per-wave time of one sequential update (t_update_us) and the rate of the whole epoch over 2048 tiles"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--nnz", type=int, default=10000000)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("fold_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    V, D, E = a.vocab, a.dim, a.epochs
    coo = capi.synth_coo(V, 10 * V, seed=0xC0FFEE)
    I, J, X, _, xmax = coo.get()
    cfg = config(D)
    h = geglove.Adagrad(geglove.CooMatrix(V, I, J, X, xmax), cfg, cfg.costFunction())
    coo.close()
    del I, J, X
    h.epoch(0)

    new = capi.synth_coo(V, a.nnz, rows=(0, a.rows), seed=0xF01D)
    nI, nJ, nX, _, _ = new.get()
    order = np.argsort(nI, kind="stable")
    row_ptr = np.concatenate(([0], np.cumsum(np.bincount(nI, minlength=a.rows)[:a.rows]))).astype(np.int64)
    idx, Xs = np.ascontiguousarray(nJ[order]), np.ascontiguousarray(nX[order])
    new.close()
    lens = np.diff(row_ptr)
    longest = int(np.argmax(lens))

    f = capi.Folding(h._h, row_ptr, idx, Xs, side="focus", epochs=E, shuffle="device", seed=7)
    info = f.info
    ms = timed(f, a.reps)
    _, _, cost, history = f.run()
    f.close()
    lo, hi = int(row_ptr[longest]), int(row_ptr[longest + 1])
    one = capi.Folding(h._h, [0, hi - lo], idx[lo:hi], Xs[lo:hi], side="focus", epochs=E, shuffle="device", seed=7)
    ms_one = timed(one, a.reps)
    one.close()
    gbps = C.c_double()
    capi.check(capi.lib().ge_copy_bandwidth(0, 1 << 30, 5, C.byref(gbps)))
    h.close()

    med, med_one = statistics.median(ms), statistics.median(ms_one)
    updates = info["nnz"] * E
    bytes_read = updates * (D * 4 + 20)
    doc = {"tool": "tests/tools/fold_bench.py", "command": "python " + " ".join(["tests/tools/fold_bench.py"] + sys.argv[1:]),
           "V": V, "dim": D, "new_rows": info["n_rows"], "nnz": info["nnz"], "epochs": E, "side": "focus",
           "shuffle": "device", "row_length_median_max": [int(np.median(lens)), int(lens.max())],
           "kernel_ms": round(med, 3), "kernel_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "reps": a.reps,
           "updates": updates, "updates_per_s": round(updates / (med * 1e-3)),
           "bytes_read_by_the_updates": bytes_read, "rate_gb_per_s": round(bytes_read / (med * 1e-3) / 1e9, 1),
           "copy_bandwidth_gb_per_s": round(gbps.value, 1), "rate_over_copy_bandwidth": round(bytes_read / (med * 1e-3) / 1e9 / gbps.value, 3),
           "path": info["path"], "longest_row_alone_ms": round(med_one, 3),
           "longest_row_alone_us_per_update": round(med_one * 1e3 / info["path"], 4),
           "longest_row_share_of_the_time": round(med_one / med, 3),
           "cost_history_first_last": [float(history[0]), float(history[-1])], "all_costs_finite": bool(np.all(np.isfinite(cost))),
           "strata_fp32_yardstick": yardstick(), "counters_taken": False}
    print(json.dumps(doc), flush=True)
    if a.out:
        with open(a.out, "w") as out:
            json.dump(doc, out, indent=1)
            out.write("\n")


if __name__ == "__main__":
    main()

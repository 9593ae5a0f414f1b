"""The held-out evaluation pass at the flagship scale.
    python tests/tools/eval_bench.py [--cases f32:625000:125000000:200,bf16:625000:125000000:300] [--fraction 0.05] [--reps 5]
                                     [--threads 16] [--no-host] [--out profiles/eval_bench.json]

A case is dtype:V:nnz:dim.  The matrix is ge_synth_coo's (generated on the device, brought down once); ge_holdout_mask splits it;
a HOGWILD handle trains two epochs on the kept nonzeros; a ge_eval holds the held-out ones.  Per case, all in this one process:
  * device time of ge_glove_eval_run (ge_eval_last_kernel_ms: hipEvents around its two kernels): one warm-up call, then --reps
    calls; median, min, max.  No outputs are copied in the timed calls (cost_sum only).
  * the bytes the pass must read, n x (2 x row bytes + 12), the rate that gives, and ge_copy_bandwidth measured here beside it;
    whether creation reordered the set by focus row, and how many distinct focus rows the set has (a sorted set re-reads a focus
    row from cache, so the bytes that must come from memory are fewer than the bytes the pass reads);
  * the same handle's epoch kernel time per nonzero (ge_glove_last_kernel_ms, the median of epochs 1 and 2);
  * the route the library offered before: four ge_glove_get_state calls plus the numpy model (float32 products, sequential
    float32 sum over d, fp64 rest; numpy log / power) on --threads threads, wall clock, once; its sum against the device's.
No counters are taken here.  One JSON document on stdout, and in --out."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
import ctypes as C                   # noqa: E402
import numpy as np                   # noqa: E402
import geglove                       # noqa: E402
from geglove import capi             # noqa: E402


def config(dim, dtype):
    return geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": dim, "threads": 1,
                                  "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                  "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                  "device": {"mode": "hogwild", "shuffle": "device", "seed": 42, "dtype": dtype}})


def host_route(handle, D, I, J, X, xmax, threads):
    """What a user had before: the four tables through ge_glove_get_state, then numpy.  Returns (seconds of the copies, seconds of
    the arithmetic, cost_sum in the partition of the header)."""
    t0 = time.perf_counter()
    focus = handle.get_state("focus").reshape(-1, D); context = handle.get_state("context").reshape(-1, D)
    fbias = handle.get_state("fbias"); cbias = handle.get_state("cbias")
    t1 = time.perf_counter()

    def block(b0):
        i, j, x = I[b0:b0 + 1024], J[b0:b0 + 1024], X[b0:b0 + 1024]
        prod = focus[i] * context[j]
        s = np.zeros(len(i), np.float32)
        for d in range(D):
            s = s + prod[:, d]
        xd = x.astype(np.float64)
        w = np.where(xd > xmax, np.float32(1.0), np.power(xd / xmax, 0.75).astype(np.float32)).astype(np.float32)
        ic = (s.astype(np.float64) + ((fbias[i] + cbias[j]).astype(np.float64) - np.log(xd))).astype(np.float32)
        t = (0.5 * (w * ic).astype(np.float64)) * ic.astype(np.float64)
        sb = 0.0
        for v in t.tolist():
            sb = sb + v
        return sb
    with ThreadPoolExecutor(threads) as pool:
        sums = list(pool.map(block, range(0, len(I), 1024), chunksize=64))
    total = 0.0
    for sb in sums:
        total = total + sb
    return t1 - t0, time.perf_counter() - t1, total


def bench(case, fraction, reps, threads, with_host):
    dtype, V, nnz, D = case.split(":")
    V, nnz, D = int(V), int(nnz), int(D)
    coo = capi.synth_coo(V, nnz, seed=0xC0FFEE)
    I, J, X, _, xmax = coo.get()
    coo.close()
    held = capi.holdout_mask(42, nnz, fraction).astype(bool)
    kI, kJ, kX = I[~held], J[~held], X[~held]
    hI, hJ, hX = np.ascontiguousarray(I[held]), np.ascontiguousarray(J[held]), np.ascontiguousarray(X[held])
    del I, J, X
    n = int(hI.shape[0])
    line = {"case": case, "dtype": dtype, "V": V, "nnz": nnz, "dim": D, "fraction": fraction, "n_held": n, "n_kept": int(kI.shape[0])}
    cfg = config(D, dtype)
    t0 = time.perf_counter()
    h = geglove.Adagrad(geglove.CooMatrix(V, kI, kJ, kX, xmax), cfg, cfg.costFunction())
    line["trainer_create_s"] = round(time.perf_counter() - t0, 2)
    epoch_ms = []
    for it in range(3):
        h.epoch(it)
        if it > 0:
            epoch_ms.append(h.last_kernel_ms()[0])
    t0 = time.perf_counter()
    ev = capi.Evaluation(h._h, hI, hJ, hX)
    line["eval_create_s"] = round(time.perf_counter() - t0, 3)
    ev.run(residual=False, term=False)                                   # warm-up
    ms, wall, total = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, _, total = ev.run(residual=False, term=False)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ev.kernel_ms())
    gbps = C.c_double()
    capi.check(capi.lib().ge_copy_bandwidth(0, 1 << 30, 5, C.byref(gbps)))
    row_bytes = D * (2 if dtype == "bf16" else 4)
    must_read = n * (2 * row_bytes + 12)
    distinct_focus = int(np.unique(hI).shape[0])
    med = statistics.median(ms)
    e_med = statistics.median(epoch_ms)
    line.update({
        "eval_kernel_ms": round(med, 3), "eval_kernel_ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "reps": reps,
        "eval_call_wall_ms": round(statistics.median(wall), 3),
        "bytes_read_by_the_pass": must_read, "row_bytes": row_bytes,
        "rate_gb_per_s": round(must_read / (med * 1e-3) / 1e9, 1),
        "copy_bandwidth_gb_per_s": round(gbps.value, 1), "rate_over_copy_bandwidth": round(must_read / (med * 1e-3) / 1e9 / gbps.value, 3),
        "set_reordered_at_creation": ev.reordered(), "set_sorted_by_focus_row": bool(np.all(np.diff(hI) >= 0)),
        "distinct_focus_rows": distinct_focus,
        "bytes_from_memory_if_focus_rows_are_reused": n * (row_bytes + 12) + distinct_focus * row_bytes,
        "eval_ns_per_nonzero": round(med * 1e6 / n, 3),
        "epoch_kernel_ms": round(e_med, 3), "epoch_ns_per_nonzero": round(e_med * 1e6 / int(kI.shape[0]), 3),
        "eval_over_epoch_per_nonzero": round((med / n) / (e_med / int(kI.shape[0])), 3),
        "mean_heldout_cost": total / n, "counters_taken": False})
    if with_host:
        copy_s, math_s, host_total = host_route(h, D, hI, hJ, hX, xmax, threads)
        line.update({"host_route_copy_s": round(copy_s, 3), "host_route_numpy_s": round(math_s, 3), "host_route_threads": threads,
                     "host_route_over_device_call": round((copy_s + math_s) * 1e3 / statistics.median(wall), 1),
                     "host_route_sum_relative_difference": abs(host_total - total) / abs(total)})
    ev.close(); h.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f32:625000:125000000:200,bf16:625000:125000000:300")
    ap.add_argument("--fraction", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("eval_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    doc = {"tool": "tests/tools/eval_bench.py", "cases": []}
    for case in [c for c in a.cases.split(",") if c]:
        doc["cases"].append(bench(case, a.fraction, a.reps, a.threads, not a.no_host))
        print(json.dumps(doc["cases"][-1]), flush=True)
        if a.out:                                        # after every case: a later case that fails leaves the earlier ones on record
            with open(a.out, "w") as f:
                json.dump(doc, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

"""Clustering stage throughput: Lloyd steps on the device next to the nearest-neighbour score kernel and to numpy.
    python tests/tools/kmeans_bench.py [--cases 300050x200:256,5000000x200:1024,1000000x300:64] [--reps 5] [--max-iter 30]
                                       [--out profiles/kmeans_bench.json]

A case is  rows x dim : K.  The table is K planted centres on the unit sphere plus noise (so that a run converges), clustered
under cosine from the keyed initial sample.  One JSON line per case: the device time of a step's assign (k_km_assign and the
objective's block sums) and update (the member sort, k_km_piece_sums, k_km_centroids), hipEvents around the kernels, median of
`reps` steps after one warm-up step, with the spread; the fp32 matrix rate of the assign, counting 2 n K dim; the steps
ge_kmeans_run then needs to converge (at most --max-iter in all).  Beside them two yardsticks taken in the same process:
k_nn_score_select at k = 1 over the same table with K queries -- the same tile and the same 2 n K dim with a heavier epilogue --
measured as tests/tools/nn_bench.py measures it; and one Lloyd iteration in numpy (fp32 X @ C.T, argmax, a sorted segment sum) on
`--cpu-rows` of the rows with the thread count the environment sets, scaled to all rows."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
from geglove import capi            # noqa: E402

PEAK_F32_MATRIX_TF = 155.0


def planted_table(n, D, K, noise=0.6, seed=1):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((K, D), dtype=np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = np.empty((n, D), np.float32)
    for b in range(0, n, 1 << 18):
        e = min(n, b + (1 << 18))
        X[b:e] = centres[rng.integers(0, K, e - b)] + (noise / np.sqrt(D)) * rng.standard_normal((e - b, D), dtype=np.float32)
    return X


def numpy_lloyd(X, C):
    """One iteration on the rows X: normalise, fp32 scores, argmax, per-cluster sums through a stable sort; seconds."""
    t0 = time.perf_counter()
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    label = np.argmax(Xn @ C.T, axis=1)
    order = np.argsort(label, kind="stable")
    starts = np.searchsorted(label[order], np.arange(C.shape[0]))
    S = np.add.reduceat(Xn[order].astype(np.float64), np.minimum(starts, len(order) - 1), axis=0)
    S /= np.maximum(np.linalg.norm(S, axis=1, keepdims=True), 1e-300)
    return time.perf_counter() - t0


def nn_yardstick(X, K, reps):
    """k_nn_score_select at k = 1: K queries against every row, device ms of the query call as nn_bench.py takes them."""
    queries = np.sort(np.random.default_rng(2).choice(X.shape[0], K, replace=False)).astype(np.int32)
    nn = capi.Neighbors.create(X)
    ms = []
    for rep in range(reps + 1):
        nn.query_rows(queries, 1)
        if rep:
            ms.append(nn.kernel_ms()[1])
    nn.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="300050x200:256,5000000x200:1024,1000000x300:64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--cpu-rows", type=int, default=50000)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    L = capi.lib()
    if L.ge_device_count() <= 0:
        raise SystemExit("kmeans_bench needs a gfx950 device: " + L.ge_last_error().decode())
    for case in a.cases.split(","):
        shape, K = case.split(":")
        n, D = (int(v) for v in shape.split("x"))
        K = int(K)
        X = planted_table(n, D, K)
        t0 = time.perf_counter()
        km = capi.Clustering.create(X, K, seed=1)
        create_s = time.perf_counter() - t0
        first = km.centroids
        assign, update, changed = [], [], []
        for rep in range(a.reps + 1):
            ch, _ = km.step()
            changed.append(ch)
            if rep:                                             # the first step warms up
                am, um = km.kernel_ms
                assign.append(am); update.append(um)
        steps, converged = a.reps + 1, changed[-1] == 0
        if not converged and a.max_iter > steps:
            more, converged = km.run(a.max_iter - steps)
            steps += more
        km.close()
        a_s = statistics.median(assign) * 1e-3
        tf = 2.0 * n * K * D / a_s / 1e12
        nn_ms = nn_yardstick(X, K, a.reps)
        nn_tf = 2.0 * n * K * D / (statistics.median(nn_ms) * 1e-3) / 1e12
        line = {"n": n, "dim": D, "k": K, "metric": "cosine", "reps": a.reps, "create_call_s": round(create_s, 2),
                "assign_device_ms": round(a_s * 1e3, 3), "assign_device_ms_min_max": [round(min(assign), 3), round(max(assign), 3)],
                "update_device_ms": round(statistics.median(update), 3), "update_device_ms_min_max": [round(min(update), 3), round(max(update), 3)],
                "assign_fp32_tflops": round(tf, 2), "share_of_155_tf": round(tf / PEAK_F32_MATRIX_TF, 3),
                "changed_per_step": changed, "steps": steps, "converged": bool(converged), "max_iter": a.max_iter,
                "nn_k1_query_device_ms": round(statistics.median(nn_ms), 3), "nn_k1_query_device_ms_min_max": [round(min(nn_ms), 3), round(max(nn_ms), 3)],
                "nn_k1_fp32_tflops": round(nn_tf, 2)}
        if not a.no_cpu:
            rows = min(n, a.cpu_rows)
            cpu_s = numpy_lloyd(X[:: max(1, n // rows)][:rows], first)
            line.update({"numpy_rows_timed": rows, "numpy_iteration_s_timed": round(cpu_s, 3), "numpy_iteration_s_scaled_to_all": round(cpu_s * n / rows, 1),
                         "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()})
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del X


if __name__ == "__main__":
    main()

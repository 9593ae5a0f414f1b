"""PCA stage throughput: the moment pass and the projection on the device next to numpy in fp64 on the host's cores.
    python tests/tools/pca_bench.py [--shapes 300050x200,5000000x200,5000000x300] [--reps 5] [--out profiles/pca_bench.json]

One JSON line per shape: the device time of the moment pass (k_pca_gram + its reduction) and of the projection (k_pca_project),
hipEvents around the kernels, median of `reps` calls after one warm-up call; the host time of the eigen solve; the fp64 FLOP/s
of the Gram kernel counting n D (D + 1); the GB/s of both kernels (the table read once; the projection also writes n k floats)
beside ge_copy_bandwidth measured in the same process; and the time numpy's fp64 X.T @ X and projection take on this host with the
thread count the environment sets (blocks of rows, the widening to fp64 included)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
from geglove import capi            # noqa: E402


def table(n, D, ratio=0.97, seed=1):
    """Column variances falling geometrically (k at 0.95 is about 100), a small offset; generated in blocks."""
    rng = np.random.default_rng(seed)
    s = (ratio ** (np.arange(D) / 2.0)).astype(np.float32)
    X = np.empty((n, D), np.float32)
    for b in range(0, n, 1 << 18):
        e = min(n, b + (1 << 18))
        X[b:e] = rng.standard_normal((e - b, D), dtype=np.float32) * s + np.float32(0.3)
    return X


def numpy_baseline(X, mean, Wk):
    n, D = X.shape
    t0 = time.perf_counter()
    G = np.zeros((D, D))
    for b in range(0, n, 1 << 18):
        blk = X[b:b + (1 << 18)].astype(np.float64)
        G += blk.T @ blk
    t1 = time.perf_counter()
    out = np.empty((n, Wk.shape[1]), np.float32)
    for b in range(0, n, 1 << 18):
        out[b:b + (1 << 18)] = (X[b:b + (1 << 18)].astype(np.float64) - mean) @ Wk
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="300050x200,5000000x200,5000000x300")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    L = capi.lib()
    if L.ge_device_count() <= 0:
        raise SystemExit("pca_bench needs a gfx950 device: " + L.ge_last_error().decode())
    gbps = C.c_double()
    capi.check(L.ge_copy_bandwidth(0, 1 << 30, 10, C.byref(gbps)))
    for shape in a.shapes.split(","):
        n, D = (int(v) for v in shape.split("x"))
        X = table(n, D)
        fit_ms, tr_ms, fit_wall, tr_wall = [], [], [], []
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            p = capi.Pca.fit(X)
            t1 = time.perf_counter()
            out = p.transform(X)
            t2 = time.perf_counter()
            if rep:                                             # the first call warms up
                f, t = p.kernel_ms()
                fit_ms.append(f); tr_ms.append(t); fit_wall.append(t1 - t0); tr_wall.append(t2 - t1)
            if rep < a.reps:
                p.close()
        _, k, _, mean, cov, lam, W = p.get()
        t0 = time.perf_counter()
        capi.Pca.from_moments(mean, cov, n).close()
        eig_s = time.perf_counter() - t0
        fit_s, tr_s = statistics.median(fit_ms) * 1e-3, statistics.median(tr_ms) * 1e-3
        line = {"n": n, "dim": D, "k": k, "reps": a.reps,
                "moments_device_ms": round(fit_s * 1e3, 3), "project_device_ms": round(tr_s * 1e3, 3), "eigen_host_ms": round(eig_s * 1e3, 3),
                "moments_call_ms": round(statistics.median(fit_wall) * 1e3, 1), "project_call_ms": round(statistics.median(tr_wall) * 1e3, 1),
                "gram_fp64_tflops": round(n * D * (D + 1) / fit_s / 1e12, 3),
                "gram_gbps": round(n * D * 4 / fit_s / 1e9, 1), "project_gbps": round((n * D * 4 + n * k * 4) / tr_s / 1e9, 1),
                "project_fp32_tflops": round(2.0 * n * D * k / tr_s / 1e12, 3),
                "copy_gbps": round(gbps.value, 1)}
        if not a.no_cpu:
            g_s, p_s = numpy_baseline(X, mean, W[:, :k])
            line.update({"numpy_gram_s": round(g_s, 3), "numpy_project_s": round(p_s, 3),
                         "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()})
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del X, out
        p.close()


if __name__ == "__main__":
    main()

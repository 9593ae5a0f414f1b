"""Nearest-neighbour stage throughput: index preparation and top-k queries on the device next to numpy on the host.
    python tests/tools/nn_bench.py [--cases 300050x200:all:10,5000000x200:10000:10,1000000x300:10000:10] [--reps 5] [--out profiles/nn_bench.json]

A case is  rows x dim : queries (a number of them, or `all` for every row with exclude_self) : k.  One JSON line per case: the
device time of the index preparation (k_nn_prepare) and of a query call (k_nn_score_select + k_nn_merge), hipEvents around the
kernels, median of `reps` calls after one warm-up call; the wall time of the same calls (uploads and downloads included); the fp32
matrix rate the query achieves, counting 2 nq n dim, and its share of the 155 TF the fp32 matrix cores measure; and the time the
same work takes in numpy on this host with the thread count the environment sets: blocked fp32 Q @ X.T plus argpartition on
`--cpu-queries` of the queries, scaled to all of them (the full all-pairs product would take the host many minutes)."""
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


def table(n, D, seed=1):
    rng = np.random.default_rng(seed)
    X = np.empty((n, D), np.float32)
    for b in range(0, n, 1 << 18):
        e = min(n, b + (1 << 18))
        X[b:e] = rng.standard_normal((e - b, D), dtype=np.float32)
    return X


def numpy_baseline(X, queries, k, block=1 << 17):
    """Normalise, then per block of candidates fp32 Q @ X.T and argpartition, keeping a running best k; seconds."""
    t0 = time.perf_counter()
    Xn = X / np.linalg.norm(X, axis=1, keepdims=True)
    Q = Xn[queries]
    t1 = time.perf_counter()
    best_s = np.full((len(queries), k), -np.inf, np.float32)
    best_i = np.zeros((len(queries), k), np.int64)
    for b in range(0, X.shape[0], block):
        S = Q @ Xn[b:b + block].T
        kk = min(k, S.shape[1])
        part = np.argpartition(-S, kk - 1, axis=1)[:, :kk]
        s = np.concatenate([best_s, np.take_along_axis(S, part, axis=1)], axis=1)
        i = np.concatenate([best_i, part + b], axis=1)
        keep = np.argpartition(-s, k - 1, axis=1)[:, :k]
        best_s, best_i = np.take_along_axis(s, keep, axis=1), np.take_along_axis(i, keep, axis=1)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="300050x200:all:10,5000000x200:10000:10,1000000x300:10000:10")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--cpu-queries", type=int, default=256)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    L = capi.lib()
    if L.ge_device_count() <= 0:
        raise SystemExit("nn_bench needs a gfx950 device: " + L.ge_last_error().decode())
    for case in a.cases.split(","):
        shape, nq_text, k = case.split(":")
        n, D = (int(v) for v in shape.split("x"))
        k = int(k)
        X = table(n, D)
        every = nq_text == "all"
        queries = None if every else np.sort(np.random.default_rng(2).choice(n, int(nq_text), replace=False)).astype(np.int32)
        nq = n if every else len(queries)
        prep_ms, query_ms, prep_wall, query_wall = [], [], [], []
        t0 = time.perf_counter()
        nn = capi.Neighbors.create(X)
        prep_wall.append(time.perf_counter() - t0)
        prep_ms.append(nn.kernel_ms()[0])
        for rep in range(a.reps + 1):
            t0 = time.perf_counter()
            idx, score = nn.query_rows(queries, k, exclude_self=every)
            t1 = time.perf_counter()
            if rep:                                             # the first call warms up
                query_ms.append(nn.kernel_ms()[1]); query_wall.append(t1 - t0)
        nn.close()
        for rep in range(2):                                    # the preparation twice more (the table goes up again each time)
            t0 = time.perf_counter()
            nn = capi.Neighbors.create(X)
            prep_wall.append(time.perf_counter() - t0)
            prep_ms.append(nn.kernel_ms()[0])
            nn.close()
        q_s = statistics.median(query_ms) * 1e-3
        tf = 2.0 * nq * n * D / q_s / 1e12
        line = {"n": n, "dim": D, "queries": nq, "k": k, "exclude_self": every, "reps": a.reps,
                "prepare_device_ms": round(statistics.median(prep_ms), 3), "prepare_call_ms": round(statistics.median(prep_wall) * 1e3, 1),
                "query_device_ms": round(q_s * 1e3, 3), "query_device_ms_min_max": [round(min(query_ms), 3), round(max(query_ms), 3)],
                "query_call_ms": round(statistics.median(query_wall) * 1e3, 1),
                "query_fp32_tflops": round(tf, 2), "share_of_155_tf": round(tf / PEAK_F32_MATRIX_TF, 3)}
        if not a.no_cpu:
            sample = np.arange(n) if every else queries
            sample = sample[:: max(1, len(sample) // a.cpu_queries)][:a.cpu_queries]
            norm_s, q_cpu_s = numpy_baseline(X, sample, k)
            line.update({"numpy_queries_timed": len(sample), "numpy_normalise_s": round(norm_s, 3), "numpy_query_s_timed": round(q_cpu_s, 3),
                         "numpy_query_s_scaled_to_all": round(q_cpu_s * nq / len(sample), 1),
                         "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()})
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del X, idx, score


if __name__ == "__main__":
    main()

"""Prediction throughput next to its yardstick, the nearest-neighbour query at the same K, in one process on
one table.
    python tests/tools/predict_bench.py [--rows 300050] [--dim 200] [--queries 10000] [--filter 100] [--k 10 100] [--reps 5]
                                        [--out profiles/predict_bench.json]

The setting of rank_bench.py: a Hogwild fp32 handle gets the table of nn_bench.py as its focus AND its context table through
ge_glove_set_state, and uniform column biases.  `queries` rows with filter lists of about `filter` ids are predicted
(ge_glove_predict_run); the same rows are then the queries of ge_nn_query_rows at the same K, metric dot, over the same vectors:
the same 64 x 128 score tile and the same lists, without the bias, the filter test and the staging.  Per K one warm-up call of
each, then `reps` timed calls, the two alternating; device time from hipEvents around the kernels, median with min - max.  Both
matrix rates count 2 * queries * rows * dim; prediction's is given over the select kernel alone (what the yardstick's tile is
compared with) and over all three phases.  One JSON line per K."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geglove                      # noqa: E402
from geglove import capi            # noqa: E402
from nn_bench import table, PEAK_F32_MATRIX_TF      # noqa: E402
from rank_bench import rank_set, spread             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300050)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--filter", type=int, default=100)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    V, D, n = a.rows, a.dim, a.queries
    I, _, ptr, idx = rank_set(V, n, a.filter)
    X = table(V, D)
    cbias = np.random.default_rng(3).uniform(-1.0, 1.0, V).astype(np.float32)
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("predict_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())

    rows = np.arange(V, dtype=np.int32)                         # the handle's own matrix: one nonzero per row, never trained
    cfg = geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": D, "threads": 1,
                                 "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                 "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                 "device": {"mode": "hogwild", "shuffle": "device", "seed": 42}})
    h = geglove.createOptimizer(cfg, geglove.CooMatrix(V, rows, rows[::-1].copy(), np.full(V, 0.05, np.float32), 0.2))
    h.set_state("focus", X); h.set_state("context", X); h.set_state("cbias", cbias)
    pr = capi.Prediction(h._h, I, (ptr, idx))
    nn = capi.Neighbors.create(X, metric="dot")

    work = 2.0 * n * V * D
    tf = lambda ms: work / (ms * 1e-3) / 1e12
    lines = []
    for K in a.k:
        phases, nn_ms = [], []
        for rep in range(a.reps + 1):                           # the first call of each warms up
            index, score, count = pr.run(K)
            nn_index, _ = nn.query_rows(I, K)
            if rep:
                phases.append(pr.kernel_ms()); nn_ms.append(nn.kernel_ms()[1])
        stage, select, merge = (spread([p[i] for p in phases]) for i in range(3))
        total = spread([sum(p) for p in phases])
        yard = spread(nn_ms)
        filtered = sum(int(np.isin(index[q, :count[q]], idx[ptr[q]:ptr[q + 1]]).any()) for q in range(0, n, 97))
        lines.append({"rows": V, "dim": D, "queries": n, "k": K, "filter_entries": int(ptr[-1]), "ranges": pr.info()["ranges"], "reps": a.reps,
                      "stage_device_ms": stage[0], "stage_device_ms_min_max": stage[1],
                      "select_device_ms": select[0], "select_device_ms_min_max": select[1],
                      "merge_device_ms": merge[0], "merge_device_ms_min_max": merge[1],
                      "predict_device_ms": total[0], "predict_device_ms_min_max": total[1],
                      "nn_dot_device_ms": yard[0], "nn_dot_device_ms_min_max": yard[1],
                      "select_fp32_tflops": round(tf(select[0]), 2), "predict_fp32_tflops": round(tf(total[0]), 2), "nn_fp32_tflops": round(tf(yard[0]), 2),
                      "select_share_of_155_tf": round(tf(select[0]) / PEAK_F32_MATRIX_TF, 3),
                      "select_time_over_nn_time": round(select[0] / yard[0], 3), "predict_time_over_nn_time": round(total[0] / yard[0], 3),
                      "all_lists_full": bool(np.all(count == K)), "sampled_queries_listing_a_filtered_column": filtered})
    nn.close(); pr.close(); h.close()
    for line in lines:
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()

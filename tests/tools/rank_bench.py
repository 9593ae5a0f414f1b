"""Ranking throughput next to its yardstick, the nearest-neighbour query at k = 1, in one process on one table.
    python tests/tools/rank_bench.py [--rows 300050] [--dim 200] [--pairs 10000] [--filter 100] [--reps 5] [--out profiles/rank_bench.json]

A Hogwild fp32 handle gets the table of nn_bench.py as its focus AND its context table through ge_glove_set_state, and uniform
column biases.  `pairs` (row, column) pairs with filter lists of about `filter` ids are ranked (ge_glove_rank_run); the rows of
the same pairs are then the queries of ge_nn_query_rows at k = 1, metric dot, over the same vectors: the same 64 x 128 score tile
with the cheapest selection.  One warm-up call of each, then `reps` timed calls, the two alternating; device time from hipEvents
around the kernels, median with min - max.  Both matrix rates count 2 * pairs * rows * dim; the ranking's is given over the count
kernel alone (what the yardstick's tile is compared with) and over all three phases.  One JSON line."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geglove                      # noqa: E402
from geglove import capi            # noqa: E402
from nn_bench import table, PEAK_F32_MATRIX_TF      # noqa: E402


def rank_set(rows, pairs, per_list, seed=2):
    """Sorted distinct rows, any columns, and per pair a strictly ascending list of about per_list ids."""
    rng = np.random.default_rng(seed)
    I = np.sort(rng.choice(rows, pairs, replace=False)).astype(np.int32)
    J = rng.integers(0, rows, pairs).astype(np.int32)
    lists = [np.unique(rng.integers(0, rows, per_list)).astype(np.int32) for _ in range(pairs)]
    ptr = np.zeros(pairs + 1, np.int64)
    ptr[1:] = np.cumsum([len(l) for l in lists])
    return I, J, ptr, np.concatenate(lists) if per_list else np.zeros(0, np.int32)


def spread(ms):
    return round(statistics.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300050)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--filter", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    V, D, n = a.rows, a.dim, a.pairs
    I, J, ptr, idx = rank_set(V, n, a.filter)
    X = table(V, D)
    cbias = np.random.default_rng(3).uniform(-1.0, 1.0, V).astype(np.float32)
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("rank_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())

    rows = np.arange(V, dtype=np.int32)                         # the handle's own matrix: one nonzero per row, never trained
    cfg = geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": D, "threads": 1,
                                 "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                 "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                 "device": {"mode": "hogwild", "shuffle": "device", "seed": 42}})
    h = geglove.createOptimizer(cfg, geglove.CooMatrix(V, rows, rows[::-1].copy(), np.full(V, 0.05, np.float32), 0.2))
    h.set_state("focus", X); h.set_state("context", X); h.set_state("cbias", cbias)
    rk = capi.Ranking(h._h, I, J, ptr, idx)
    nn = capi.Neighbors.create(X, metric="dot")

    phases, nn_ms = [], []
    for rep in range(a.reps + 1):                               # the first call of each warms up
        rank, _, summary = rk.run()
        index, _ = nn.query_rows(I, 1)
        if rep:
            phases.append(rk.phase_ms()); nn_ms.append(nn.kernel_ms()[1])
    nn.close(); rk.close(); h.close()

    work = 2.0 * n * V * D
    stage, gather, count = (spread([p[i] for p in phases]) for i in range(3))
    total = spread([sum(p) for p in phases])
    yard = spread(nn_ms)
    tf = lambda ms: work / (ms * 1e-3) / 1e12
    line = {"rows": V, "dim": D, "pairs": n, "filter_entries": int(ptr[-1]), "reps": a.reps,
            "stage_device_ms": stage[0], "stage_device_ms_min_max": stage[1],
            "gather_device_ms": gather[0], "gather_device_ms_min_max": gather[1],
            "count_device_ms": count[0], "count_device_ms_min_max": count[1],
            "rank_device_ms": total[0], "rank_device_ms_min_max": total[1],
            "nn_k1_dot_device_ms": yard[0], "nn_k1_dot_device_ms_min_max": yard[1],
            "count_fp32_tflops": round(tf(count[0]), 2), "rank_fp32_tflops": round(tf(total[0]), 2), "nn_fp32_tflops": round(tf(yard[0]), 2),
            "count_share_of_155_tf": round(tf(count[0]) / PEAK_F32_MATRIX_TF, 3),
            "count_rate_over_nn_rate": round(yard[0] / count[0], 3), "rank_rate_over_nn_rate": round(yard[0] / total[0], 3),
            "mrr": summary["mrr"], "mean_rank": summary["mean_rank"], "nn_top1_is_the_query_row": float(np.mean(index[:, 0] == I))}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""The threshold join next to the exact neighbour index: join, sort and components time, in one process.
    python tests/tools/match_bench.py [--rows 300050] [--dim 200] [--planted 0.1] [--noise 0.02] [--threshold 0.9]
                                      [--pairs 10000000] [--reps 5] [--k 10] [--out profiles/match_bench.json]

The table: --rows random unit rows of --dim, of which the last --planted share are noisy copies of the first ones (copy =
original + --noise * a fresh unit direction).  Random 200-d rows have cosines of order 0.07, so at T = 0.9 only planted pairs
qualify; the pair count is recorded next to the planted number.
  * ge_match_run at --threshold: join, sort and components device time (hipEvents, median of --reps runs after a warm-up run,
    with the spread), the host clock around the call, the pairs found and the summary;
  * the yardstick: ge_nn_query_rows over all rows with k = --k and exclude_self on the same table in the same process (device
    time, median of --reps after a warm-up), and join / query;
  * a second line at a threshold low enough for about --pairs pairs (taken from a sample of the table's scores), to show what the
    write path, the sort and the components cost."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from geglove import capi             # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def table(n, dim, planted, noise, seed=11):
    rng = np.random.default_rng(seed)
    copies = int(round(n * planted))
    X = rng.standard_normal((n, dim)).astype(np.float32)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    E = rng.standard_normal((copies, dim)).astype(np.float32)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    X[n - copies:] = X[:copies] + np.float32(noise) * E
    return X, copies


def timed(m, T, cap, reps):
    m.run(T, cap)                                                                            # warm-up
    join, sort, comp, wall = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        a, b, s, label, summary = m.run(T, cap)
        wall.append((time.perf_counter() - t0) * 1e3)
        _, j, so, c = m.kernel_ms()
        join.append(j); sort.append(so); comp.append(c)
    return {"threshold": T, "max_pairs": cap, "summary": summary, "join_ms": spread(join), "sort_ms": spread(sort), "components_ms": spread(comp),
            "host_call_ms": spread(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300050)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--pairs", type=int, default=10 ** 7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_bench.json"))
    a = ap.parse_args()
    assert capi.lib().ge_device_count() > 0, "match_bench measures on the device: no gfx950 device visible"

    X, copies = table(a.rows, a.dim, a.planted, a.noise)
    n = X.shape[0]
    out = {"tool": "tests/tools/match_bench.py", "n": n, "dim": a.dim, "metric": "cosine", "planted_pairs": copies, "noise": a.noise, "reps": a.reps}
    m = capi.Matching.from_rows(X)
    out["prepare_ms"] = round(m.kernel_ms()[0], 3)
    out["planted"] = timed(m, a.threshold, 1 << 24, a.reps)
    # the products the join computes: every (query tile, candidate tile) it walks is 64 x 128 x D4 fused multiply-adds
    D4 = (a.dim + 3) // 4 * 4
    qtiles, ctiles = (n + 63) // 64, (n + 127) // 128
    tiles = sum(ctiles - (64 * qt + 1) // 128 for qt in range(qtiles))
    out["join_tflops"] = round(2.0 * tiles * 64 * 128 * D4 / (out["planted"]["join_ms"]["median"] * 1e-3) / 1e12, 2)

    nn = capi.Neighbors.create(X)
    nn.query_rows(None, a.k, exclude_self=True)                                              # warm-up
    q = []
    for _ in range(a.reps):
        nn.query_rows(None, a.k, exclude_self=True)
        q.append(nn.kernel_ms()[1])
    nn.close()
    out["nn_query_rows"] = {"k": a.k, "query_ms": spread(q), "tflops": round(2.0 * n * n * D4 / (statistics.median(q) * 1e-3) / 1e12, 2)}
    out["join_over_query"] = round(out["planted"]["join_ms"]["median"] / statistics.median(q), 4)

    # a threshold for about --pairs pairs: the matching quantile of the scores of a sample of rows against each other
    rng = np.random.default_rng(5)
    pick = np.sort(rng.choice(n, size=min(n, 4000), replace=False))
    Y = X[pick].astype(np.float64)
    Y /= np.linalg.norm(Y, axis=1, keepdims=True)
    S = (Y @ Y.T)[np.triu_indices(pick.size, 1)]
    share = a.pairs / (n * (n - 1) / 2.0)
    T2 = float(np.float32(np.quantile(S, 1.0 - share)))
    out["many_pairs"] = timed(m, T2, 1 << 25, a.reps)
    m.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""The inverted-file index next to the exact one: build time, query time and recall, in one process.
    python tests/tools/ivf_bench.py [--rows 1000000] [--dim 200] [--lists 0] [--iterations 10] [--probes 1,4,16,64] [--k 10]
                                    [--reps 5] [--recall-queries 10000] [--tables planted,trained] [--out profiles/ivf_bench.json]

Two tables of --rows x --dim: `planted` = nn_ref.planted clusters (1000 rows each, noise 1.0), and `trained` = the vectors of a
HOGWILD handle trained for three epochs on a ge_synth_coo matrix of 10 nonzeros per row (indexed through ge_glove_ivf_create /
ge_glove_nn_create).  L = --lists, or sqrt(rows) rounded to a power of two.  Per table:
  * the build: the host clock around ge_ivf_create (training included), around ge_kmeans_create + ge_kmeans_run alone (the training
    phase, run once more on its own), and the device time of the index's own kernels (prepare, assign, sort, gather);
  * per nprobe: probe, scan and merge device time of an all-rows query with exclude_self (hipEvents, median of --reps calls after
    a warm-up call, with the spread), the host clock around the call, mean and maximum of out_candidates, and recall@k against
    ge_nn_query_rows on --recall-queries keyed-sampled rows;
  * the device time of ge_nn's exact all-rows query (median of --reps after a warm-up) -- the yardstick for quality and time --
    and exact / IVF at every nprobe."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import geglove                       # noqa: E402
from geglove import capi, synth      # noqa: E402
import nn_ref                        # noqa: E402


def trainer(V, D):
    coo = capi.synth_coo(V, 10 * V, seed=0xC0FFEE)
    I, J, X, _, xmax = coo.get()
    cfg = geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": D, "threads": 1,
                                 "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                 "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                 "device": {"mode": "hogwild", "shuffle": "device", "seed": 42}})
    h = geglove.Adagrad(geglove.CooMatrix(V, I, J, X, xmax), cfg, cfg.costFunction())
    coo.close()
    for it in range(3):
        h.epoch(it)
    return h


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def bench(name, n, D, L, T, probes, k, reps, nrecall):
    handle, X = None, None
    if name == "planted":
        X, _ = nn_ref.planted(7, n // 1000, 1000, D, noise=1.0)
        n = X.shape[0]
    else:
        handle = trainer(n, D)
    out = {"table": name, "n": n, "dim": D, "lists": L, "train_iterations": T, "k": k, "reps": reps}

    t0 = time.perf_counter()
    ivf = capi.IvfNeighbors.create(X, L, train_iterations=T, seed=1) if handle is None else capi.IvfNeighbors.create_glove(handle._h, L, train_iterations=T, seed=1)
    out["create_call_s"] = round(time.perf_counter() - t0, 3)
    g = ivf.get()
    sizes = ivf.sizes
    out.update({"train_steps": g["train_steps"], "converged": g["converged"], "build_device_ms": round(ivf.kernel_ms()[0], 3),
                "list_size_mean_max_empty": [round(float(sizes.mean()), 1), int(sizes.max()), int((sizes == 0).sum())]})
    t0 = time.perf_counter()
    km = capi.Clustering.create(X, L, seed=1) if handle is None else capi.Clustering.create_glove(handle._h, L, seed=1)
    km.run(T)
    out["train_alone_call_s"] = round(time.perf_counter() - t0, 3)
    km.close()

    nn = capi.Neighbors.create(X) if handle is None else capi.Neighbors.create_glove(handle._h)
    exact_ms = []
    for rep in range(reps + 1):
        nn.query_rows(None, k, exclude_self=True)
        if rep:
            exact_ms.append(nn.kernel_ms()[1])
    out["exact_query_device_ms"] = spread(exact_ms)
    ids = np.sort(np.argsort(synth.splitmix64(99, n), kind="stable")[:nrecall]).astype(np.int32)
    truth, _ = nn.query_rows(ids, k, exclude_self=True)
    nn.close()

    out["probes"] = []
    for P in probes:
        if P > min(L, 128):
            continue
        ms, wall = {"probe": [], "scan": [], "merge": []}, []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            _, _, count, cand = ivf.query_rows(None, k, P, exclude_self=True)
            t1 = time.perf_counter()
            if rep:
                _, p, s, m = ivf.kernel_ms()
                ms["probe"].append(p); ms["scan"].append(s); ms["merge"].append(m); wall.append(t1 - t0)
        got, _, _, _ = ivf.query_rows(ids, k, P, exclude_self=True)
        hit = sum(len(np.intersect1d(a, b)) for a, b in zip(got, truth))
        total = statistics.median([a + b + c for a, b, c in zip(ms["probe"], ms["scan"], ms["merge"])])
        out["probes"].append({"nprobe": P, "probe_device_ms": spread(ms["probe"]), "scan_device_ms": spread(ms["scan"]), "merge_device_ms": spread(ms["merge"]),
                              "query_device_ms": round(total, 3), "query_call_ms": round(statistics.median(wall) * 1e3, 1),
                              "candidates_mean_max": [round(float(cand.mean()), 1), int(cand.max())], "short_results": int((count < k).sum()),
                              "recall_at_k": round(hit / (len(ids) * k), 4), "recall_queries": len(ids),
                              "exact_over_ivf": round(statistics.median(exact_ms) / total, 2), "lists_over_nprobe": round(L / P, 1)})
        print(json.dumps(out["probes"][-1]), flush=True)
    ivf.close()
    if handle is not None:
        handle.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--lists", type=int, default=0)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--probes", default="1,4,16,64")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--recall-queries", type=int, default=10000)
    ap.add_argument("--tables", default="planted,trained")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("ivf_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    L = a.lists or 1 << round(math.log2(math.sqrt(a.rows)))
    cases = []
    for name in a.tables.split(","):
        cases.append(bench(name, a.rows, a.dim, L, a.iterations, [int(p) for p in a.probes.split(",")], a.k, a.reps, a.recall_queries))
        print(json.dumps({key: v for key, v in cases[-1].items() if key != "probes"}), flush=True)
        if a.out:                                                       # after every table: a later one that fails loses nothing
            with open(a.out, "w") as f:
                json.dump({"tool": "tests/tools/ivf_bench.py", "cases": cases}, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()

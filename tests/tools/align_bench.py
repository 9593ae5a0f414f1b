"""The rectangular join and the one-to-one assignment next to the detour through ge_match_* (DESIGN.md 3.16), in one process.
    python tests/tools/align_bench.py [--rows 300050] [--dim 200] [--planted 0.1] [--noise 0.02] [--threshold 0.9]
                                      [--pairs 10000000] [--reps 5] [--out profiles/align_bench.json]

The table is match_bench.py's: --rows random unit rows of --dim, of which the last --planted share are noisy copies of the first
ones.  The first half of the rows is the source set, the second half the target set, so every planted pair crosses the two sets.
  * ge_align_run at --threshold: join, sort and assign device time (hipEvents, median of --reps runs after a warm-up run, with
    the spread), the assignment rounds, the host clock around the call, and the summary;
  * the detour: ge_match_run over all rows at the same threshold in the same process (its join time, median of --reps after a
    warm-up), and align join / match join;
  * a second line at a threshold low enough for about --pairs candidates (taken from a sample of the table's cross scores), to
    show what the write path, the three sorts and the rounds cost."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
from geglove import capi             # noqa: E402
from match_bench import spread, table   # noqa: E402


def timed(al, T, cap, reps):
    al.run(T, cap)                                                                           # warm-up
    join, sort, assign, wall = [], [], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        summary = al.run(T, cap)[7]
        wall.append((time.perf_counter() - t0) * 1e3)
        _, j, so, asg, rounds = al.kernel_ms()
        join.append(j); sort.append(so); assign.append(asg)
    return {"threshold": T, "max_pairs": cap, "summary": summary, "rounds": rounds, "join_ms": spread(join), "sort_ms": spread(sort),
            "assign_ms": spread(assign), "host_call_ms": spread(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300050)
    ap.add_argument("--dim", type=int, default=200)
    ap.add_argument("--planted", type=float, default=0.1)
    ap.add_argument("--noise", type=float, default=0.02)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--pairs", type=int, default=10 ** 7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    a = ap.parse_args()
    assert capi.lib().ge_device_count() > 0, "align_bench measures on the device: no gfx950 device visible"

    X, copies = table(a.rows, a.dim, a.planted, a.noise)
    n = X.shape[0]
    source, target = np.arange(0, n // 2, dtype=np.int32), np.arange(n // 2, n, dtype=np.int32)
    assert copies <= source.size and copies <= target.size                                   # every planted pair crosses the sets
    out = {"tool": "tests/tools/align_bench.py", "n": n, "n_source": int(source.size), "n_target": int(target.size), "dim": a.dim, "metric": "cosine",
           "planted_pairs": copies, "noise": a.noise, "reps": a.reps}
    al = capi.Alignment.from_rows(X, source, target)
    out["prepare_ms"] = round(al.kernel_ms()[0], 3)
    out["planted"] = timed(al, a.threshold, 1 << 24, a.reps)
    # the products the join computes: every (query tile, candidate tile) of the rectangle is 64 x 128 x D4 fused multiply-adds
    D4 = (a.dim + 3) // 4 * 4
    tiles = ((source.size + 63) // 64) * ((target.size + 127) // 128)
    out["join_tflops"] = round(2.0 * tiles * 64 * 128 * D4 / (out["planted"]["join_ms"]["median"] * 1e-3) / 1e12, 2)

    m = capi.Matching.from_rows(X)
    m.run(a.threshold, 1 << 24)                                                              # warm-up
    q = []
    for _ in range(a.reps):
        m.run(a.threshold, 1 << 24)
        q.append(m.kernel_ms()[1])
    m.close()
    out["match_union"] = {"join_ms": spread(q)}
    out["join_over_match_join"] = round(out["planted"]["join_ms"]["median"] / statistics.median(q), 4)

    # a threshold for about --pairs candidates: the matching quantile of the cross scores of a sample of both sets
    rng = np.random.default_rng(5)
    pa = np.sort(rng.choice(source, size=min(source.size, 3000), replace=False))
    pb = np.sort(rng.choice(target, size=min(target.size, 3000), replace=False))
    A, B = X[pa].astype(np.float64), X[pb].astype(np.float64)
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    share = a.pairs / (float(source.size) * float(target.size))
    T2 = float(np.float32(np.quantile((A @ B.T).ravel(), 1.0 - share)))
    out["many_candidates"] = timed(al, T2, 1 << 25, a.reps)
    al.close()

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()

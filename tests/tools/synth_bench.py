"""The on-device generator next to the host recipe.
    python tests/tools/synth_bench.py [--cases c2,shard,c4] [--reps 5] [--no-host] [--no-trainer] [--out profiles/synth_bench.json]

c2 = BASELINE C2's shape: V = 100 000, all rows, nnz 10^7;  shard = the bench shard: V = 5 000 000, rows [0, 625 000), nnz 125 000 000;  c4 = BASELINE C4 whole on one GPU: V = 5 000 000, all
rows, nnz 10^9.  One JSON line per case.  Every figure is the median of `reps` calls after one warm-up call:
  generate_device_ms   ge_coo_synth_stats: hipEvents around the generator's kernels, sorts and scans
  generate_call_ms     host clock around ge_synth_coo (allocations included; the call returns with the stream drained)
  draws, peak_bytes    what the generator consumed and the most device memory it held
and for c2 and the shard also
  host_recipe_s        geglove.synth.synthetic_coo_shard for the same shard on this machine's CPU -- the figure the generator is set
                       against (another recipe: fp64 pow, de-duplicated to fewer than the named nnz)
  create_coo_ms / create_arrays_ms   ge_glove_create_coo on the device-resident matrix and ge_glove_create on the arrays ge_coo_get
                       returned, dim 200, with the laps GE_GLOVE_TIMING=1 prints (the upload lap is what the in-place route loses)
  epoch_ms             the epoch kernel at dim 200 on the generated shard (recorded only: not the bench's matrix)
Which kernel or sort dominates comes from a run of its own:  rocprofv3 --kernel-trace --stats -- python tests/tools/synth_bench.py
--cases shard --reps 1 --no-host --no-trainer."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
import geglove                       # noqa: E402
from geglove import capi, synth      # noqa: E402

CASES = {"c2": (100_000, (0, 100_000), 10_000_000), "shard": (5_000_000, (0, 625_000), 125_000_000), "c4": (5_000_000, (0, 5_000_000), 1_000_000_000)}
med = statistics.median


def stderr_of(fn):
    """fn() with file descriptor 2 redirected: (result, what the library printed)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            out = fn()
        finally:
            os.dup2(saved, 2); os.close(saved)
        f.seek(0)
        return out, f.read().decode(errors="replace")


def laps(text):
    return {m.group(1).strip(): float(m.group(2)) for m in re.finditer(r"\[ge_glove_create\]\s+(.*?)\s+([0-9.]+) ms", text)}


def generate(V, rows, nnz, reps):
    dev_ms, call_ms, draws, peak = [], [], 0, 0
    coo = None
    for rep in range(reps + 1):
        if coo is not None:
            coo.close()
        t0 = time.perf_counter()
        coo = capi.synth_coo(V, nnz, rows=rows)
        t1 = time.perf_counter()
        draws, ms, peak = coo.stats()
        if rep:                                                 # the first call warms up
            dev_ms.append(ms); call_ms.append((t1 - t0) * 1e3)
    M = nnz - (rows[1] - rows[0])
    line = {"generate_device_ms": round(med(dev_ms), 2), "generate_device_ms_min_max": [round(min(dev_ms), 2), round(max(dev_ms), 2)],
            "generate_call_ms": round(med(call_ms), 1), "draws": draws, "draws_per_key": round(draws / M, 4),
            "peak_bytes": peak, "peak_bytes_per_nonzero": round(peak / nnz, 2),
            "nonzeros_per_second_device": round(nnz / (med(dev_ms) * 1e-3), 0)}
    return coo, line


def trainer(coo, V, rows, reps):
    I, J, X, row_ptr, mx = coo.get()
    host = geglove.CooMatrix(V, I, J, X, mx)
    dev = geglove.DeviceCooMatrix(coo)
    cfg = geglove.Configuration({"graph": "synthetic", "method": "glove", "dim": 200, "threads": 1,
                                 "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                 "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                 "device": {"seed": 42, "row_range": rows}})
    os.environ["GE_GLOVE_TIMING"] = "1"
    out = {}
    for name, m in (("create_coo", dev), ("create_arrays", host)):
        wall, lap_list = [], []
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            opt, text = stderr_of(lambda: geglove.Adagrad(m, cfg, cfg.costFunction()))
            t1 = time.perf_counter()
            if rep:
                wall.append((t1 - t0) * 1e3); lap_list.append(laps(text))
            if rep < reps or name == "create_arrays":
                opt.close()
        out[name + "_ms"] = round(med(wall), 1)
        out[name + "_laps_ms"] = {k: round(med([l[k] for l in lap_list if k in l]), 2) for k in lap_list[0]}
        if name == "create_coo":
            keep = opt
    del os.environ["GE_GLOVE_TIMING"]
    ms = []
    for it in range(reps + 1):
        cost = keep.epoch(it)
        if it:
            ms.append(keep.last_kernel_ms()[0])
    out.update({"epoch_dim": 200, "epoch_ms": round(med(ms), 2), "epoch_ms_min_max": [round(min(ms), 2), round(max(ms), 2)],
                "epoch_cost_per_nonzero_last": cost / len(I), "workers": keep.info()["groups_in_flight"], "hot_columns": keep.info()["hot_columns"]})
    keep.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c2,shard,c4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-trainer", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("synth_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    for case in a.cases.split(","):
        V, rows, nnz = CASES[case]
        coo, line = generate(V, rows, nnz, a.reps)
        line = dict({"case": case, "V": V, "rows": list(rows), "nnz": nnz, "reps": a.reps}, **line)
        if case != "c4" and not a.no_trainer:
            line.update(trainer(coo, V, rows, a.reps))
        coo.close()
        if case != "c4" and not a.no_host:
            t = []
            for rep in range(a.reps + 1):
                t0 = time.perf_counter()
                I, J, X, xmax = synth.synthetic_coo_shard(V, rows, nnz, seed=0xC0FFEE)
                if rep:
                    t.append(time.perf_counter() - t0)
            line.update({"host_recipe_s": round(med(t), 2), "host_recipe_nonzeros": int(len(I)),
                         "host_threads": int(os.environ.get("OMP_NUM_THREADS", 0)) or os.cpu_count()})
            del I, J, X
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()

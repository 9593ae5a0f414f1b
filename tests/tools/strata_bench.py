"""The stratified trainer mode beside the one-wave mode and Hogwild.
    python tests/tools/strata_bench.py [--cases c3,c2] [--strata 128,256,512,1024,2048] [--epochs 10] [--det-epochs 2]
                                       [--exact] [--exact-strata 0] [--out profiles/strata_bench.json]

c3 = the C3 stand-in: synth.dblp_like_graph at 50 040 vertices -> ge_bca_build -> pglove, dim 200.
c2 = BASELINE C2: 100 k vertices, 10 M nonzeros, glove, dim 100.
Per case every handle lives in this one process on the same matrix and the epochs ALTERNATE: round `it` runs epoch `it` of every
stratified handle (one per P) and of the Hogwild handle; the one-wave handle (GE_MODE_DETERMINISTIC, shuffle none, threads 1) joins
the first --det-epochs rounds only (its epoch takes seconds).  Epoch 0 of every handle warms up; the times are the device-event
times of ge_glove_last_kernel_ms over the remaining epochs: median, min, max.  Reported per handle: ms per epoch, updates / s,
strata_path / N, launches, the ratio to the one-wave epoch, and the mean cost per nonzero of epochs 1 .. epochs-1 next to Hogwild's
over the same epochs.
--exact: two stratified epochs (shuffle device) of the C3 stand-in against the oracle replaying ge_glove_epoch_order: all eight
tables must be bit-equal and the extracted vectors within 1e-4 (asserted; the oracle takes tens of seconds per epoch).
One JSON document on stdout, and in --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np                   # noqa: E402
import geglove                       # noqa: E402
from geglove import capi, synth      # noqa: E402


def config(dim, method, **device):
    return geglove.Configuration({"graph": "synthetic", "method": method, "dim": dim, "threads": 1,
                                  "bca": {"alpha": 0.1, "epsilon": 1e-3, "directed": True},
                                  "opt": {"method": "adagrad", "tolerance": 0, "maxiter": 1}, "output": {"uri": []},
                                  "device": dict(device, seed=42)})


def matrix(case):
    if case == "c3":
        g = synth.dblp_like_graph(10000, 15000, 40)
        m = geglove.BookmarkColoring(g, config(200, "pglove"))
        return m, 200, "pglove"
    V = 100_000
    I, J, X, xmax = synth.synthetic_coo_shard(V, (0, V), 12_100_000, seed=0xC0FFEE)       # de-duplicated: 10.0 M remain
    return geglove.CooMatrix(V, I, J, X, xmax), 100, "glove"


def summary(ms):
    return {"ms_per_epoch": round(statistics.median(ms), 3), "ms_min_max": [round(min(ms), 3), round(max(ms), 3)], "timed_epochs": len(ms)}


def bench(case, strata, epochs, det_epochs):
    m, D, method = matrix(case)
    N, V = m.coOccurrenceCount(), m.vocabSize()
    cols = np.bincount(m.J, minlength=V)
    line = {"case": case, "V": V, "nnz": N, "dim": D, "method": method, "busiest_column_share": round(float(cols.max()) / N, 6),
            "epochs": epochs, "det_epochs": det_epochs}
    handles = []
    for P in strata:
        t0 = time.perf_counter()
        h = geglove.Adagrad(m, config(D, method, mode="stratified", strata=P, shuffle="device"), config(D, method).costFunction())
        handles.append(("P%d" % P, h, (time.perf_counter() - t0) * 1e3))
    hog = geglove.Adagrad(m, config(D, method, mode="hogwild", shuffle="device"), config(D, method).costFunction())
    det = geglove.Adagrad(m, config(D, method, mode="deterministic", shuffle="none"), config(D, method).costFunction())
    ms = {name: [] for name, _, _ in handles}; ms["hogwild"] = []; ms["one_wave"] = []
    cost = {name: [] for name in ms}
    launches = {}
    for it in range(epochs):
        for name, h, _ in handles + [("hogwild", hog, 0.0)] + ([("one_wave", det, 0.0)] if it < det_epochs else []):
            c = h.epoch(it)
            t, n = h.last_kernel_ms()
            launches[name] = n
            cost[name].append(c / N)
            if it > 0 or name == "one_wave":            # epoch 0 warms up (the one-wave epoch runs for seconds: its launch is noise)
                ms[name].append(t)
    one = statistics.median(ms["one_wave"])
    hog_mean = float(np.mean(cost["hogwild"][1:]))
    line["one_wave"] = dict(summary(ms["one_wave"]), updates_per_s=round(N / (one * 1e-3)), cost_per_nonzero=cost["one_wave"])
    line["hogwild"] = dict(summary(ms["hogwild"]), updates_per_s=round(N / (statistics.median(ms["hogwild"]) * 1e-3)),
                           mean_cost_epochs_1_on=hog_mean, workers=hog.info()["groups_in_flight"])
    line["stratified"] = []
    for name, h, create_ms in handles:
        info = h.info()
        med = statistics.median(ms[name])
        line["stratified"].append(dict(summary(ms[name]), strata=info["strata"], strata_path=info["strata_path"],
                                       path_over_n=round(info["strata_path"] / N, 6), launches=launches[name],
                                       updates_per_s=round(N / (med * 1e-3)), us_per_path_update=round(med * 1e3 / max(info["strata_path"], 1), 3),
                                       speedup_over_one_wave=round(one / med, 2), create_ms=round(create_ms, 1),
                                       mean_cost_epochs_1_on=float(np.mean(cost[name][1:])),
                                       mean_cost_over_hogwild=round(float(np.mean(cost[name][1:])) / hog_mean, 5)))
        h.close()
    best = min(line["stratified"], key=lambda r: r["ms_per_epoch"])
    line["fastest_strata"] = best["strata"]
    line["default_strata"] = geglove.Adagrad(m, config(D, method, mode="stratified", shuffle="device"), config(D, method).costFunction()).info()["strata"]
    line["stratified_faster_than_one_wave"] = bool(best["ms_per_epoch"] < one)
    hog.close(); det.close()
    return line


def exact(P):
    """Two stratified epochs of the C3 stand-in against the oracle replaying the reported order."""
    import oracle as O
    m, D, method = matrix("c3")
    V, N = m.vocabSize(), m.coOccurrenceCount()
    I, J, X = np.ascontiguousarray(m.I), np.ascontiguousarray(m.J), np.ascontiguousarray(m.X)
    dev = geglove.Adagrad(m, config(D, method, mode="stratified", strata=P, shuffle="device"), config(D, method).costFunction())
    ref = {k: np.ascontiguousarray(v.reshape(V, -1) if v.size == V * D else v, np.float32) for k, v in dev.state().items()}
    out = {"case": "c3", "V": V, "nnz": N, "dim": D, "strata": dev.info()["strata"], "epochs": 2, "oracle_s": [], "device_ms": []}
    for it in range(2):
        order = dev.epoch_order(it).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(N))
        dev.epoch(it)
        out["device_ms"].append(round(dev.last_kernel_ms()[0], 2))
        t0 = time.perf_counter()
        O.adagrad_job(D, I[order], J[order], X[order], m.max(), O.COST_PGLOVE, ref)
        out["oracle_s"].append(round(time.perf_counter() - t0, 1))
    got = dev.state()
    differing = {k: int(np.count_nonzero(got[k].reshape(-1).view(np.uint32) != ref[k].reshape(-1).view(np.uint32))) for k in ref}
    vec = dev.extractResultF32().reshape(V, D)
    want = (ref["focus"] + ref["context"]) / np.float32(2.0)
    out["tables_bit_equal"] = all(v == 0 for v in differing.values())
    out["words_differing"] = differing
    out["vectors_max_abs_diff"] = float(np.max(np.abs(vec.astype(np.float64) - want.astype(np.float64))))
    dev.close()
    assert out["tables_bit_equal"], differing
    assert out["vectors_max_abs_diff"] <= 1e-4, out["vectors_max_abs_diff"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c2")
    ap.add_argument("--strata", default="128,256,512,1024,2048")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--det-epochs", type=int, default=2)
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--exact-strata", type=int, default=0, help="P of the --exact run (0 = the library default)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("strata_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    doc = {"tool": "tests/tools/strata_bench.py", "cases": [], "exact": None}
    strata = [int(x) for x in a.strata.split(",") if x]
    for case in [c for c in a.cases.split(",") if c]:
        doc["cases"].append(bench(case, strata, a.epochs, a.det_epochs))
        print(json.dumps(doc["cases"][-1]), flush=True)
    if a.exact:
        doc["exact"] = exact(a.exact_strata)
        print(json.dumps(doc["exact"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

"""The stratified trainer's two arithmetics side by side: GE_ARITH_JAVA (k_adagrad_strata) and GE_ARITH_FP32
(k_strata_fp32) on the same matrix, the same P, the same schedule.
    python tests/tools/strata_fp32_bench.py [--cases c3,c2] [--strata 512,1024,2048] [--epochs 10] [--no-ablation]
                                            [--out profiles/strata_fp32_bench.json]

The method is tests/tools/strata_bench.py's, and so are the matrices (c3 = the C3 stand-in, pglove, dim 200; c2 = BASELINE C2,
glove, dim 100).  Per case every handle lives in this one process and the epochs ALTERNATE: round `it` runs epoch `it` of, for every
P, the java handle, the fp32 handle and (unless --no-ablation) two more fp32 handles that run with GE_STRATA_FP32_ABLATE = 1 (no
prefetch) and = 2 (no prefetch, no forwarding), and of one Hogwild handle.  Epoch 0 of every handle warms up; the times are the
device-event times of ge_glove_last_kernel_ms over the remaining epochs: median, min, max.  Reported per (case, P) and handle:
ms per epoch, ms per epoch / strata_path (the effective time of one sequential update, t_update), the mean cost per nonzero of
epochs 1 .. epochs-1 (next to Hogwild's), and java's ms over fp32's.  The ablated handles must reproduce the fp32 handle's costs to
the bit (asserted): neither the prefetch nor the forwarding is part of the result.
One JSON document on stdout, and in --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "graph-embeddings_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                   # noqa: E402
import geglove                       # noqa: E402
from geglove import capi             # noqa: E402
from strata_bench import config, matrix, summary      # noqa: E402

ABLATE = "GE_STRATA_FP32_ABLATE"
VARIANTS = (("java", "java", None), ("fp32", "fp32", None), ("fp32_no_prefetch", "fp32", "1"), ("fp32_no_prefetch_no_forwarding", "fp32", "2"))


def bench(case, strata, epochs, ablation):
    m, D, method = matrix(case)
    N, V = m.coOccurrenceCount(), m.vocabSize()
    line = {"case": case, "V": V, "nnz": N, "dim": D, "method": method, "epochs": epochs}
    variants = [v for v in VARIANTS if ablation or v[2] is None]
    handles = []                      # (P, name, handle, ablate)
    for P in strata:
        for name, arith, ablate in variants:
            h = geglove.Adagrad(m, config(D, method, mode="stratified", arith=arith, strata=P, shuffle="device"), config(D, method).costFunction())
            handles.append((P, name, h, ablate))
    hog = geglove.Adagrad(m, config(D, method, mode="hogwild", shuffle="device"), config(D, method).costFunction())
    ms = {(P, name): [] for P, name, _, _ in handles}
    cost = {(P, name): [] for P, name, _, _ in handles}
    hog_ms, hog_cost = [], []
    for it in range(epochs):
        for P, name, h, ablate in handles:
            if ablate is None:
                os.environ.pop(ABLATE, None)
            else:
                os.environ[ABLATE] = ablate
            c = h.epoch(it)
            os.environ.pop(ABLATE, None)
            cost[(P, name)].append(c / N)
            if it > 0:                # epoch 0 warms up
                ms[(P, name)].append(h.last_kernel_ms()[0])
        hog_cost.append(hog.epoch(it) / N)
        if it > 0:
            hog_ms.append(hog.last_kernel_ms()[0])
    line["hogwild"] = dict(summary(hog_ms), mean_cost_epochs_1_on=float(np.mean(hog_cost[1:])))
    line["strata"] = []
    for P in strata:
        hs = {name: h for p, name, h, _ in handles if p == P}
        info = hs["java"].info()
        assert hs["fp32"].get_arith() == capi.GE_ARITH_FP32 and hs["java"].get_arith() == capi.GE_ARITH_JAVA
        path = max(info["strata_path"], 1)
        row = {"strata": info["strata"], "strata_path": info["strata_path"], "path_over_n": round(info["strata_path"] / N, 6)}
        for name in hs:
            med = statistics.median(ms[(P, name)])
            row[name] = dict(summary(ms[(P, name)]), t_update_us=round(med * 1e3 / path, 4), updates_per_s=round(N / (med * 1e-3)),
                             mean_cost_epochs_1_on=float(np.mean(cost[(P, name)][1:])))
            if name.startswith("fp32_"):
                assert cost[(P, name)] == cost[(P, "fp32")], (case, P, name, "an ablated run changed the result")
        row["java_ms_over_fp32_ms"] = round(row["java"]["ms_per_epoch"] / row["fp32"]["ms_per_epoch"], 2)
        row["fp32_faster_than_java"] = bool(row["fp32"]["ms_per_epoch"] < row["java"]["ms_per_epoch"])
        row["fp32_mean_cost_over_java"] = round(row["fp32"]["mean_cost_epochs_1_on"] / row["java"]["mean_cost_epochs_1_on"], 7)
        row["fp32_mean_cost_over_hogwild"] = round(row["fp32"]["mean_cost_epochs_1_on"] / line["hogwild"]["mean_cost_epochs_1_on"], 5)
        line["strata"].append(row)
    for _, _, h, _ in handles:
        h.close()
    hog.close()
    line["fastest_fp32_strata"] = min(line["strata"], key=lambda r: r["fp32"]["ms_per_epoch"])["strata"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c2")
    ap.add_argument("--strata", default="512,1024,2048")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--no-ablation", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if capi.lib().ge_device_count() <= 0:
        raise SystemExit("strata_fp32_bench needs a gfx950 device: " + capi.lib().ge_last_error().decode())
    doc = {"tool": "tests/tools/strata_fp32_bench.py", "device": "MI355X (gfx950)", "cases": []}
    strata = [int(x) for x in a.strata.split(",") if x]
    for case in [c for c in a.cases.split(",") if c]:
        doc["cases"].append(bench(case, strata, a.epochs, not a.no_ablation))
        print(json.dumps(doc["cases"][-1]), flush=True)
    doc["fp32_faster_than_java_everywhere"] = all(r["fp32_faster_than_java"] for c in doc["cases"] for r in c["strata"])
    print(json.dumps({"fp32_faster_than_java_everywhere": doc["fp32_faster_than_java_everywhere"]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

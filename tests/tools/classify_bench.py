"""Classification throughput: the loss-and-gradient evaluation of ge_classify_* next to the same loss and
gradient written in torch, and a whole fit.
    python tests/tools/classify_bench.py [--cases 1000000x200:16,1000000x200:256] [--reps 5] [--max-iter 60]
                                         [--out profiles/classify_bench.json]

A case is  rows x dim : C.  The table is C planted centres on the unit sphere plus noise; every row is labelled with its centre
and every row trains.  One JSON line per case: the device time of one evaluation's three phases (k_cls_logits; k_cls_softmax
with the loss block sums; k_cls_gradient with the piece sums), hipEvents around the kernels as ge_classify_last_kernel_ms
reports them, median of `reps` evaluations at seeded weights after one warm-up, with the spread; the bytes the model of an
evaluation moves (the feature table twice, z and r written and read once each) and the rate they give; the fp32 matrix rate of
the two products (2 n C Dp each); then a whole fit from zero weights: iterations, evaluations, stop reason, wall seconds.
Beside them, in the same process, the same loss and gradient in torch on the same device (matmul, log_softmax, matmul, fp32),
timed with device events the same way: the outside yardstick."""
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


def planted_table(n, D, C, noise=0.8, seed=1):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D), dtype=np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    X = np.empty((n, D), np.float32)
    y = rng.integers(0, C, n).astype(np.int32)
    for b in range(0, n, 1 << 18):
        e = min(n, b + (1 << 18))
        X[b:e] = centres[y[b:e]] + (noise / np.sqrt(D)) * rng.standard_normal((e - b, D), dtype=np.float32)
    return X, y


def torch_yardstick(X, y, W, l2, reps):
    """The same f and g in torch, fp32 on the device: (median ms, min, max, loss)."""
    import torch
    dev = torch.device("cuda")
    Xn = torch.from_numpy(X).to(dev)
    Xn = Xn / Xn.norm(dim=1, keepdim=True)
    XH = torch.cat([Xn, torch.ones(Xn.shape[0], 1, device=dev)], dim=1).contiguous()
    del Xn
    yt = torch.from_numpy(y.astype(np.int64)).to(dev)
    Wt = torch.from_numpy(W).to(dev)
    rows = torch.arange(XH.shape[0], device=dev)
    ms, loss = [], None
    for rep in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        Z = XH @ Wt.T
        logp = torch.log_softmax(Z, dim=1)
        loss = -logp[rows, yt].mean() + 0.5 * l2 * (Wt[:, :-1] ** 2).sum()
        R = torch.exp(logp)
        R[rows, yt] -= 1.0
        G = R.T @ XH / XH.shape[0]
        G[:, :-1] += l2 * Wt[:, :-1]
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms), float(loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1000000x200:16,1000000x200:256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=60)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    L = capi.lib()
    if L.ge_device_count() <= 0:
        raise SystemExit("classify_bench needs a gfx950 device: " + L.ge_last_error().decode())
    for case in a.cases.split(","):
        shape, C = case.split(":")
        n, D = (int(v) for v in shape.split("x"))
        C = int(C)
        X, y = planted_table(n, D, C)
        t0 = time.perf_counter()
        clf = capi.Classifier.create(X, y, C)
        create_s = time.perf_counter() - t0
        W = (0.1 * np.random.default_rng(3).standard_normal((C, D + 1))).astype(np.float32)
        clf.set_weights(W)
        phases, loss = [], None
        for rep in range(a.reps + 1):
            loss, _ = clf.eval()
            if rep:
                phases.append(clf.kernel_ms)
        logits, softmax, gradient = (statistics.median(p[i] for p in phases) for i in range(3))
        total = [sum(p) for p in phases]
        dp4 = (D + 1 + 3) // 4 * 4
        model_bytes = 2 * n * dp4 * 4 + 4 * n * C * 4
        flops = 2 * 2.0 * n * C * (D + 1)
        clf.set_weights(np.zeros_like(W))
        t0 = time.perf_counter()
        iterations, stop = clf.run(a.max_iter)
        fit_s = time.perf_counter() - t0
        g = clf.get()
        train = clf.score()
        clf.close()
        med = statistics.median(total)
        line = {"n": n, "dim": D, "classes": C, "normalize": "cosine", "reps": a.reps, "create_call_s": round(create_s, 2),
                "logits_device_ms": round(logits, 3), "softmax_device_ms": round(softmax, 3), "gradient_device_ms": round(gradient, 3),
                "evaluation_device_ms": round(med, 3), "evaluation_device_ms_min_max": [round(min(total), 3), round(max(total), 3)],
                "model_bytes_per_evaluation": model_bytes, "model_gb_per_s": round(model_bytes / (med * 1e-3) / 1e9, 1),
                "products_fp32_tflops": round(flops / (med * 1e-3) / 1e12, 2),
                "logits_fp32_tflops": round(0.5 * flops / (logits * 1e-3) / 1e12, 2), "gradient_fp32_tflops": round(0.5 * flops / (gradient * 1e-3) / 1e12, 2),
                "loss_at_seeded_weights": loss, "fit_iterations": iterations, "fit_evaluations": g["evaluations"], "fit_stop": stop, "fit_loss": g["loss"],
                "fit_wall_s": round(fit_s, 2), "fit_max_iter": a.max_iter, "training_accuracy": train["accuracy"]}
        if not a.no_torch:
            ms, lo, hi, tloss = torch_yardstick(X, y, W, 1e-4, a.reps)
            line.update({"torch_evaluation_device_ms": round(ms, 3), "torch_evaluation_device_ms_min_max": [round(lo, 3), round(hi, 3)],
                         "torch_loss_at_seeded_weights": tloss, "device_over_torch": round(med / ms, 2)})
        text = json.dumps(line)
        print(text, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(text + "\n")
        del X


if __name__ == "__main__":
    main()

"""Probe: the certified prefilter of pm_knn_exact against pm_knn's prefilter, and
pm_build_graph_exact against pm_build_graph, on clustered float rows.

    python tools/knn_exact_probe.py [--n 100000] [--build-n 1000000] [--runs 3] [--out FILE.json]

Kernel times are the library's own event timings (timing level 1); the two
variants alternate.  Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pacmann_amd as pm  # noqa: E402


def clustered_floats(n, d, centres, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d)).astype(np.float32)
    v = np.empty((n, d), dtype=np.float32)
    for a in range(0, n, 1 << 16):   # chunks: no [n, d] float64 temporary
        b = min(n, a + (1 << 16))
        v[a:b] = c[np.arange(a, b) % centres] + 0.1 * rng.standard_normal((b - a, d)).astype(np.float32)
    return v


def kernel_ms(ctx, name):
    return ctx.timing_get(name)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--build-n", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = pm.Context(0)
    ctx.timing(1)
    res = {"prefilter": [], "build": None}
    for d in (128, 192):
        v = clustered_floats(a.n, d, a.centres)
        pm.knn(v, v[:256], 10, ctx)          # warm-up of both forms
        pm.knn_exact(v, v[:256], 10, ctx)
        row = {"n": a.n, "nq": a.n, "dim": d, "k": 10, "knn_prefilter_ms": [], "knn_prefilter_x3_ms": [],
               "knn_brute_ms": [], "fallback_rows": []}
        same = None
        for _ in range(a.runs):
            ctx.timing_reset()
            ids = pm.knn(v, v, 10, ctx)
            row["knn_prefilter_ms"].append(kernel_ms(ctx, "knn_prefilter"))
            ctx.timing_reset()
            ide, fb = pm.knn_exact(v, v, 10, ctx)
            row["knn_prefilter_x3_ms"].append(kernel_ms(ctx, "knn_prefilter_x3"))
            row["knn_brute_ms"].append(kernel_ms(ctx, "knn_brute"))
            row["fallback_rows"].append(fb)
            same = float((ids == ide).all(axis=1).mean())
        row["ratio"] = float(np.median(row["knn_prefilter_x3_ms"]) / np.median(row["knn_prefilter_ms"]))
        row["rows_equal_to_pm_knn"] = same
        res["prefilter"].append(row)
        print(json.dumps(row), flush=True)
    if a.build_n:
        v = clustered_floats(a.build_n, 128, a.centres)
        b = {"n": a.build_n, "dim": 128, "m": 32, "centres": a.centres}
        for name, exact in (("build_graph", False), ("build_graph_exact", True)):
            ctx.timing_reset()
            t = time.perf_counter()
            g, tm = pm.build_graph(v, 32, 1.2, seed=1, ctx=ctx, exact=exact)
            b[name] = {"wall_s": time.perf_counter() - t, **tm,
                       "prefilter_ms": kernel_ms(ctx, "knn_prefilter_x3" if exact else "knn_prefilter"),
                       "knn_rerank_ms": kernel_ms(ctx, "knn_rerank"), "knn_brute_ms": kernel_ms(ctx, "knn_brute")}
            b[name + "_rows"] = g
            print(json.dumps({name: b[name]}), flush=True)
        b["graph_rows_equal"] = float((b.pop("build_graph_rows") == b.pop("build_graph_exact_rows")).all(axis=1).mean())
        b["fallback_share"] = b["build_graph_exact"]["knn_fallback_rows"] / a.build_n
        res["build"] = b
    print(json.dumps(res))
    if a.out:
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

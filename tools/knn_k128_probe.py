"""Probe: the 128-key exact kNN (pm_knn_k128, pm_build_graph_k128) against the
unchanged 64-key kernels in the same session, on clustered float rows.

    python tools/knn_k128_probe.py [--step prefilter|build|all] [--n 100000] [--dims 128,192,256,512,768,960]
                                   [--build-n 1000000] [--runs 3] [--out FILE.json]

prefilter: per dim, pm_knn_wide (knn_prefilter_x3 up to d = 192, knn_prefilter_w
above) and pm_knn_k128 (knn_prefilter_k128, knn_prefilter_k128_w) alternate,
n = nq, k = 10; the yardstick is the 64-key kernel.  build: the n = 1,000,000,
d = 128, m = 32 build through pm_build_graph_wide and pm_build_graph_k128.
Kernel times are the library's own event timings (timing level 1).  Prints one
JSON object per row (and writes all of them to --out).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pacmann_amd as pm  # noqa: E402
from tools.knn_exact_probe import clustered_floats, kernel_ms  # noqa: E402


def prefilter_rows(ctx, a):
    out = []
    for d in (int(x) for x in a.dims.split(",")):
        wide = d > 192
        old, new = ("knn_prefilter_w", "knn_prefilter_k128_w") if wide else ("knn_prefilter_x3", "knn_prefilter_k128")
        v = clustered_floats(a.n, d, a.centres)
        pm.knn_wide(v, v[:256], 10, ctx)   # warm-up of both forms
        pm.knn_k128(v, v[:256], 10, ctx)
        row = {"n": a.n, "nq": a.n, "dim": d, "k": 10, "yardstick": old, "kernel": new}
        for form in ("64", "128"):
            for key in ("prefilter_ms", "knn_rerank_ms", "knn_brute_ms", "fallback_rows"):
                row[f"{key}_{form}"] = []
        same = True
        for _ in range(a.runs):
            ids = {}
            for form, fn, name in (("64", pm.knn_wide, old), ("128", pm.knn_k128, new)):
                ctx.timing_reset()
                ids[form], fb = fn(v, v, 10, ctx)
                row[f"prefilter_ms_{form}"].append(kernel_ms(ctx, name))
                row[f"knn_rerank_ms_{form}"].append(kernel_ms(ctx, "knn_rerank"))
                row[f"knn_brute_ms_{form}"].append(kernel_ms(ctx, "knn_brute"))
                row[f"fallback_rows_{form}"].append(fb)
            same = same and bool((ids["64"] == ids["128"]).all())
        row["ratio"] = float(np.median(row["prefilter_ms_128"]) / np.median(row["prefilter_ms_64"]))
        row["ids_equal"] = same
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def build_row(ctx, a):
    v = clustered_floats(a.build_n, 128, a.centres)
    b = {"n": a.build_n, "dim": 128, "m": 32, "centres": a.centres}
    graphs = {}
    for name, fn, pre in (("build_graph_wide", pm.build_graph_wide, "knn_prefilter_x3"),
                          ("build_graph_k128", pm.build_graph_k128, "knn_prefilter_k128")):
        ctx.timing_reset()
        t = time.perf_counter()
        graphs[name], tm = fn(v, 32, 1.2, 1, ctx)
        b[name] = {"wall_s": time.perf_counter() - t, **tm, "prefilter_ms": kernel_ms(ctx, pre),
                   "knn_rerank_ms": kernel_ms(ctx, "knn_rerank"), "knn_brute_ms": kernel_ms(ctx, "knn_brute")}
        print(json.dumps({name: b[name]}), flush=True)
    b["graph_rows_equal"] = float((graphs["build_graph_wide"] == graphs["build_graph_k128"]).all(axis=1).mean())
    print(json.dumps(b), flush=True)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("prefilter", "build", "all"))
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="128,192,256,512,768,960")
    ap.add_argument("--build-n", type=int, default=1_000_000)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = pm.Context(0)
    ctx.timing(1)
    res = {}
    if a.step in ("prefilter", "all"):
        res["prefilter"] = prefilter_rows(ctx, a)
    if a.step in ("build", "all"):
        res["build"] = build_row(ctx, a)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

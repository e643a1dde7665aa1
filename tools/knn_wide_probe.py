"""Probe: the K-chunked prefilter of pm_knn_wide (k_knn_bf16x3_w) on clustered
float rows of 256 to 960 dimensions, against the narrow k_knn_bf16x3<192> in
the same session scaled by dp / 192.

    python tools/knn_wide_probe.py [--n 100000] [--dims 256,512,768,960] [--runs 3] [--out FILE.json]

Kernel times are the library's own event timings (timing level 1).  Prints one
JSON object (and writes it to --out).
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pacmann_amd as pm  # noqa: E402
from tools.knn_exact_probe import clustered_floats, kernel_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--dims", default="256,512,768,960")
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = pm.Context(0)
    ctx.timing(1)
    res = {"n": a.n, "nq": a.n, "k": 10, "centres": a.centres, "yardstick": None, "wide": []}
    # the yardstick: k_knn_bf16x3<192> on the same box in the same session
    v = clustered_floats(a.n, 192, a.centres)
    pm.knn_exact(v, v[:256], 10, ctx)
    y = {"dim": 192, "dp": 192, "knn_prefilter_x3_ms": [], "fallback_rows": []}
    for _ in range(a.runs):
        ctx.timing_reset()
        _, fb = pm.knn_exact(v, v, 10, ctx)
        y["knn_prefilter_x3_ms"].append(kernel_ms(ctx, "knn_prefilter_x3"))
        y["fallback_rows"].append(fb)
    res["yardstick"] = y
    print(json.dumps(y), flush=True)
    base = float(np.median(y["knn_prefilter_x3_ms"]))
    for d in (int(x) for x in a.dims.split(",")):
        dp = -(-d // 64) * 64
        v = clustered_floats(a.n, d, a.centres)
        pm.knn_wide(v, v[:256], 10, ctx)   # warm-up
        row = {"dim": d, "dp": dp, "knn_prefilter_w_ms": [], "knn_rerank_ms": [], "knn_brute_ms": [],
               "fallback_rows": []}
        for _ in range(a.runs):
            ctx.timing_reset()
            _, fb = pm.knn_wide(v, v, 10, ctx)
            row["knn_prefilter_w_ms"].append(kernel_ms(ctx, "knn_prefilter_w"))
            row["knn_rerank_ms"].append(kernel_ms(ctx, "knn_rerank"))
            row["knn_brute_ms"].append(kernel_ms(ctx, "knn_brute"))
            row["fallback_rows"].append(fb)
        row["scaled_yardstick_ms"] = base * dp / 192
        row["ratio_to_scaled_yardstick"] = float(np.median(row["knn_prefilter_w_ms"]) / row["scaled_yardstick_ms"])
        res["wide"].append(row)
        print(json.dumps(row), flush=True)
    print(json.dumps(res))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

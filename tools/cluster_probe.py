"""Probe: k-means and the cluster-search baseline (pm_kmeans, pm_cluster_*) on
SIFT1M-shaped rows (pacmann_amd.synth.sift_like_vectors).

    python tools/cluster_probe.py [--n 1000000] [--dim 128] [--nc 1000] [--niter 20] [--nq 1000] [--k 10]
                                  [--nprobe 1 8 32] [--rounds 3] [--out FILE.json]

kmeans: one pm_kmeans call; per-stage kernel times (the library's own event
timings, timing level 1), the wall time, moved per assignment, and the achieved
bytes/s of "kmeans_update" against n dim 4 bytes per launch.  search: the index
from those centroids; for every nprobe the wall time per query and the kernel
times of `rounds` pm_cluster_search calls (after one warm-up), the achieved
bytes/s of "cluster_scan" against scanned dim 4 bytes, and recall@k against
pm_knn ground truth (report.compute_recall).  Prints one JSON object per row
(and writes all of them to --out).
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pacmann_amd as pm  # noqa: E402
from pacmann_amd import report  # noqa: E402
from pacmann_amd.synth import sift_like_vectors  # noqa: E402

KMEANS_NAMES = ("to_bf16", "knn_prefilter_k128", "knn_prefilter_k128_w", "knn_rerank", "knn_brute", "kmeans_sort",
                "kmeans_update", "kmeans_moved")
CREATE_NAMES = ("cluster_sort", "cluster_gather", "to_bf16")
SEARCH_NAMES = ("to_bf16", "knn_prefilter_k128", "knn_prefilter_k128_w", "knn_rerank", "knn_brute", "cluster_scan",
                "cluster_merge")


def kernels(ctx, names):
    out = {}
    for name in names:
        launches, ms, _ = ctx.timing_get(name)
        if launches:
            out[name] = {"launches": launches, "ms": ms}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nc", type=int, default=1000)
    ap.add_argument("--niter", type=int, default=20)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = pm.Context(0)
    ctx.timing(1)
    v = sift_like_vectors(a.n + a.nq, a.dim, seed=11).astype(np.float32)
    v, q = np.ascontiguousarray(v[:a.n]), np.ascontiguousarray(v[a.n:])
    res = {}

    pm.kmeans(v[:4096], 16, 2, ctx=ctx)   # warm-up
    ctx.timing_reset()
    t = time.perf_counter()
    cen, labels, sizes, moved = pm.kmeans(v, a.nc, a.niter, seed=1, ctx=ctx)
    wall = time.perf_counter() - t
    ks = kernels(ctx, KMEANS_NAMES)
    up = ks.get("kmeans_update")
    row = {"step": "kmeans", "n": a.n, "dim": a.dim, "nc": a.nc, "niter": a.niter, "wall_s": wall, "kernels": ks,
           "moved": moved.tolist(), "sizes_min_max": [int(sizes.min()), int(sizes.max())],
           "empty_clusters": int((sizes == 0).sum()),
           "kmeans_update_GBps": (up["launches"] * a.n * a.dim * 4 / (up["ms"] * 1e-3) / 1e9) if up else None}
    res["kmeans"] = row
    print(json.dumps(row), flush=True)

    ctx.timing_reset()
    t = time.perf_counter()
    idx = pm.ClusterIndex(v, cen, labels, ctx)
    row = {"step": "create", "wall_s": time.perf_counter() - t, "kernels": kernels(ctx, CREATE_NAMES)}
    res["create"] = row
    print(json.dumps(row), flush=True)

    gnd = pm.knn(v, q, a.k, ctx)
    res["search"] = []
    for nprobe in a.nprobe:
        idx.search(q, a.k, nprobe)   # warm-up
        row = {"step": "search", "nq": a.nq, "k": a.k, "nprobe": nprobe, "wall_ms_per_query": [], "kernels": []}
        for _ in range(a.rounds):
            ctx.timing_reset()
            t = time.perf_counter()
            ids, _, scanned = idx.search(q, a.k, nprobe, with_probed=True)
            row["wall_ms_per_query"].append((time.perf_counter() - t) * 1e3 / a.nq)
            row["kernels"].append(kernels(ctx, SEARCH_NAMES))
        scan_ms = float(np.median([x["cluster_scan"]["ms"] for x in row["kernels"]]))
        row["scanned_mean"] = float(scanned.mean())
        row["cluster_scan_ms"] = scan_ms
        row["cluster_scan_GBps"] = float(scanned.sum()) * a.dim * 4 / (scan_ms * 1e-3) / 1e9
        row["recall"] = float(report.compute_recall(gnd, ids, a.k))
        res["search"].append(row)
        print(json.dumps(row), flush=True)
    idx.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

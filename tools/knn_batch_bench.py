"""SearchKNNBatch (one k_knn_batch launch, pm_knnb.hip) against the per-query
SearchKNN loop on the same non-private handle, at the reference's recall-sweep
shape: SIFT-like n = 1e6, d = 128, an m = 32 graph from pm_build_graph, 10,000
queries, k = 10, 20 steps, parallel 3.

    python tools/knn_batch_bench.py [--n N] [--queries Q] [--loop-queries L] [--repeats R] [--out DIR]

The two are timed in interleaved repeats (batch, loop, batch, loop, ...) after
one untimed call of each (the first batch call uploads the graph).  The loop
runs its first L queries only and is reported as a per-query rate.  A last
batch call at timing level 1 gives the kernel's own time ("knn_batch") and its
fraction of the HBM peak over its algorithmic bytes; recall@10 is against
pm_knn.  Writes DIR/knn_batch.json and prints it.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pacmann_amd as pm  # noqa: E402
from pacmann_amd.report import compute_recall  # noqa: E402
from pacmann_amd.synth import sift_like_vectors  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X: HBM3E 8.0 TB/s spec
K, STEP, PARALLEL, M, DIM = 10, 20, 3, 32, 128


def make_queries(v, n, seed):
    rng = np.random.default_rng(seed)
    q = v[rng.integers(0, v.shape[0], size=n)] + rng.normal(0, 8, size=(n, v.shape[1])).astype(np.float32)
    return np.clip(np.rint(q), 0, 255).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--loop-queries", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "r08" / "knn_batch"))
    a = ap.parse_args()
    nl = min(a.loop_queries, a.queries)
    ctx = pm.Context(0)
    v = sift_like_vectors(a.n, DIM, seed=100)
    t = time.perf_counter()
    g, _ = pm.build_graph(v, M, 1.2, seed=1, ctx=ctx)
    build_s = time.perf_counter() - t
    qs = make_queries(v, a.queries, seed=300)
    gi = pm.PIRGraphInfo(v, g, nonprivate=True, skip_prep=True, pir_seed=1, search_seed=2, ctx=ctx)
    gi.Preprocess()

    def loop():
        return np.stack([gi.SearchKNN(q, K, STEP, PARALLEL)[0] for q in qs[:nl]])

    gi.SearchKNNBatch(qs[:nl], K, STEP, PARALLEL)   # untimed: the graph's upload
    loop_ids = loop()
    batch_s, loop_s = [], []
    for _ in range(a.repeats):
        t = time.perf_counter()
        ids, _, dq = gi.SearchKNNBatch(qs, K, STEP, PARALLEL, return_device_queries=True)
        batch_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        loop_ids = loop()
        loop_s.append(time.perf_counter() - t)
    same = bool(np.array_equal(ids[:nl], loop_ids))
    ctx.timing(1)
    ctx.timing_reset()
    gi.SearchKNNBatch(qs, K, STEP, PARALLEL)
    launches, ms, by = ctx.timing_get("knn_batch")
    _, fb_ms, _ = ctx.timing_get("host_knn_batch_fallback")
    ctx.timing(0)
    gt = pm.knn(v, qs, K, ctx)
    bq = [a.queries / s for s in batch_s]
    lq = [nl / s for s in loop_s]
    out = {
        "shape": {"n": a.n, "dim": DIM, "m": M, "queries": a.queries, "k": K, "step": STEP, "parallel": PARALLEL,
                  "loop_queries": nl, "repeats": a.repeats, "build_graph_s": round(build_s, 2)},
        "batch_call_s": [round(s, 5) for s in batch_s],
        "batch_queries_per_s": [round(x, 1) for x in bq],
        "loop_s": [round(s, 5) for s in loop_s],
        "loop_queries_per_s": [round(x, 1) for x in lq],
        "ratio_median": round(float(np.median(bq) / np.median(lq)), 1),
        "ratio_worst_batch_over_best_loop": round(min(bq) / max(lq), 1),
        "spread": {"batch": round((max(bq) - min(bq)) / float(np.median(bq)), 4),
                   "loop": round((max(lq) - min(lq)) / float(np.median(lq)), 4)},
        "device_queries": int(dq),
        "batch_equals_loop_on_loop_queries": same,
        "kernel": {"name": "knn_batch", "launches": int(launches), "ms": round(ms, 4), "alg_bytes": by,
                   "gbs": round(by / (ms * 1e-3) / 1e9, 1) if ms else None,
                   "frac_hbm_peak": round(by / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if ms else None,
                   "host_fallback_ms": round(fb_ms, 3)},
        "recall_at_10": round(float(compute_recall(gt, ids, K)), 4),
    }
    d = Path(a.out)
    d.mkdir(parents=True, exist_ok=True)
    (d / "knn_batch.json").write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

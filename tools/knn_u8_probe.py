"""Probe: the uint8 exact kNN and build (pm_knn_u8, pm_build_graph_u8) against
the float entry points in the same session, on clustered byte rows
(pacmann_amd.synth.clustered_vectors) and their float copy.

    python tools/knn_u8_probe.py [--step knn|mem|build|all] [--n 100000] [--build-n 1000000] [--rounds 3]
                                 [--out FILE.json]

knn: n = nq, d = 128, k = 10 and 100.  Form A is pm_knn_u8 ("u8_bias" +
"knn_prefilter_u8"), form B a float call on the float copy: pm_knn (k = 10 only:
"knn_prefilter" + "knn_rerank") or pm_knn_k128 ("knn_prefilter_k128" +
"knn_rerank" + "knn_brute").  Each pair runs A B B A `rounds` times.  mem: the
device bytes each call holds at its peak (pm_ctx_mem_info polled from a second
thread while the call runs, against the value before it).  build: d = 128,
m = 32 through pm_build_graph, pm_build_graph_k128 and pm_build_graph_u8.
Kernel times are the library's own event timings (timing level 1).  Prints one
JSON object per row (and writes all of them to --out).
"""
import argparse
import json
import sys
import threading
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pacmann_amd as pm  # noqa: E402
from pacmann_amd.synth import clustered_vectors  # noqa: E402

U8_NAMES = ("u8_bias", "knn_prefilter_u8")
KNN_NAMES = ("to_bf16", "knn_prefilter", "knn_rerank")
K128_NAMES = ("to_bf16", "knn_prefilter_k128", "knn_rerank", "knn_brute")


def rows(n, d):
    f = clustered_vectors(n, d, seed=11)
    b = f.astype(np.uint8)
    assert np.array_equal(b.astype(np.float32), f)
    return b, f


def kernel_ms(ctx, names):
    return {name: ctx.timing_get(name)[1] for name in names}


def forms(k):
    """name -> (call returning ids, timing names, the names summed for the comparison)"""
    f = {"knn_u8": (lambda b, v, ctx: pm.knn_u8(b, b, k, ctx), U8_NAMES, U8_NAMES),
         "knn_k128": (lambda b, v, ctx: pm.knn_k128(v, v, k, ctx)[0], K128_NAMES, K128_NAMES[1:])}
    if k <= 64:
        f["knn"] = (lambda b, v, ctx: pm.knn(v, v, k, ctx), KNN_NAMES, KNN_NAMES[1:])
    return f


def knn_rows(ctx, a):
    b, v = rows(a.n, 128)
    out = []
    for k in (10, 100):
        F = forms(k)
        for name, (call, _, _) in F.items():   # warm-up of every form
            call(b[:512], v[:512], ctx)
        for other in [x for x in F if x != "knn_u8"]:
            row = {"n": a.n, "nq": a.n, "dim": 128, "k": k, "A": "knn_u8", "B": other, "order": "ABBA" * a.rounds,
                   "A_ms": [], "B_ms": [], "A_kernels": [], "B_kernels": []}
            same = True
            ids = {}
            for _ in range(a.rounds):
                for which in "ABBA":
                    name = "knn_u8" if which == "A" else other
                    call, names, summed = F[name]
                    ctx.timing_reset()
                    ids[which] = call(b, v, ctx)
                    ms = kernel_ms(ctx, names)
                    row[f"{which}_kernels"].append(ms)
                    row[f"{which}_ms"].append(sum(ms[x] for x in summed))
                same = same and bool((ids["A"] == ids["B"]).all())
            row["ratio_A_over_B"] = float(np.median(row["A_ms"]) / np.median(row["B_ms"]))
            row["ids_equal"] = same
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def peak_bytes(ctx, call):
    """Device bytes held at the call's peak above what was held before it."""
    before = ctx.mem_info()[0]
    low = [before]
    stop = threading.Event()

    def poll():
        while not stop.is_set():
            low[0] = min(low[0], ctx.mem_info()[0])
            time.sleep(0.0005)
    t = threading.Thread(target=poll)
    t.start()
    try:
        call()
    finally:
        stop.set()
        t.join()
    return before - low[0]


def mem_rows(ctx, a):
    b, v = rows(a.n, 128)
    n, dim, dp = a.n, 128, 128
    r = {"n": n, "nq": n, "dim": dim, "k": 10,
         "derived_bytes": {"knn_u8": 2 * (n * dp + 4 * n), "knn": 2 * (n * dim * 4 + n * 128 * 2 + 4 * n),
                           "knn_k128": 2 * (n * dim * 4 + 2 * n * 128 * 2 + 4 * n)},
         "peak_bytes": {}}
    for name, (call, _, _) in forms(10).items():
        call(b[:512], v[:512], ctx)
        r["peak_bytes"][name] = [peak_bytes(ctx, lambda: call(b, v, ctx)) for _ in range(a.rounds)]
    r["float_over_u8"] = {x: float(np.median(r["peak_bytes"][x]) / np.median(r["peak_bytes"]["knn_u8"]))
                          for x in ("knn", "knn_k128")}
    print(json.dumps(r), flush=True)
    return r


def build_row(ctx, a):
    b, v = rows(a.build_n, 128)
    r = {"n": a.build_n, "dim": 128, "m": 32}
    graphs = {}
    for name, fn, x, names in (("build_graph", pm.build_graph, v, KNN_NAMES),
                               ("build_graph_k128", pm.build_graph_k128, v, K128_NAMES),
                               ("build_graph_u8", pm.build_graph_u8, b, U8_NAMES + ("u8_to_f32",))):
        ctx.timing_reset()
        t = time.perf_counter()
        graphs[name], tm = fn(x, 32, 1.2, 1, ctx)
        r[name] = {"wall_s": time.perf_counter() - t, **tm, "kernel_ms": kernel_ms(ctx, names + ("prune",))}
        print(json.dumps({name: r[name]}), flush=True)
    for other in ("build_graph", "build_graph_k128"):
        r[f"rows_equal_{other}"] = float((graphs["build_graph_u8"] == graphs[other]).all(axis=1).mean())
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=("knn", "mem", "build", "all"))
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--build-n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = pm.Context(0)
    ctx.timing(1)
    res = {}
    if a.step in ("knn", "all"):
        res["knn"] = knn_rows(ctx, a)
    if a.step in ("mem", "all"):
        res["mem"] = mem_rows(ctx, a)
    if a.step in ("build", "all"):
        res["build"] = build_row(ctx, a)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()

"""split_query_probe.py — the two-party round (pm_batchpir_client_begin ->
pm_batchpir_server_answer -> pm_batchpir_client_finish) against the one-process
step (pm_batchpir_query) on SIFT1M's batch-PIR shape: 16 partitions x 62,500
rows x 80 words, n = 96 ids per batch.

A server handle (never preprocessed) and two clients of it with one seed: A is
driven by the split round, B by Query.  Blocks run A B B A, `--batches` batches
each, on fresh ids; per block the wall time per batch of each call and the
kernel time per batch of every launch it made (timing level 2, so the step's
own kernels are timed too).  The answers of A and B must be equal.  One JSON
line at the end.  Needs the GPU; about 1.5 GB of host memory.

    timeout -k 10 300 python tools/split_query_probe.py [--batches 20]

(under a time limit, as every GPU step: the probe sets none itself; a run takes
about 10 s)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

P, ROWS, E, NIDS, F = 16, 62_500, 80, 96, 8
SPLIT_KERNELS = ("hint_match", "resolve", "client_sets", "server_answer", "client_finish")
STEP_KERNELS = ("step", "match_resolve", "hint_match", "resolve", "gather", "answer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=20, help="batches per block")
    args = ap.parse_args()
    import pacmann_amd as pm
    ctx = pm.Context(0)
    N = P * ROWS
    db = np.random.default_rng(1).integers(0, 2**64, size=N * E, dtype=np.uint64)
    server = pm.SimpleBatchPianoPIR(N, E * 8, 2 * P, db, F, seed=11, ctx=ctx)
    a, b = server.Client(5), server.Client(5)
    a.Preprocessing()
    b.Preprocessing()
    cfg = a.SubConfig(0)
    print(f"[probe] {P} partitions of {cfg['DBSize']} rows, SetSize {cfg['SetSize']}, ChunkSize {cfg['ChunkSize']}, "
          f"MaxQueryNum {cfg['MaxQueryNum']}", file=sys.stderr, flush=True)
    rng = np.random.default_rng(2)
    R = args.batches
    assert 4 * R * (NIDS // P) < cfg["MaxQueryNum"] - 8, "the blocks must stay clear of the re-preprocessing trigger"

    def kernels(names):
        return {k: round(ctx.timing_get(k)[1] / R, 4) for k in names if ctx.timing_get(k)[0]}

    def block(kind, ids):
        ctx.timing_reset()
        ctx.timing(2)
        wall = dict.fromkeys(("begin", "server", "finish", "query"), 0.0)
        outs, sets = [], 0
        for q in ids:
            t0 = time.perf_counter()
            if kind == "A":
                parts, offs = a.QueryBegin(q)
                t1 = time.perf_counter()
                ans = server.ServerAnswer(parts, offs)
                t2 = time.perf_counter()
                out, _ = a.QueryFinish(ans)
                t3 = time.perf_counter()
                wall["begin"] += t1 - t0; wall["server"] += t2 - t1; wall["finish"] += t3 - t2
                sets += len(parts)
            else:
                out, _ = b.QueryWithMask(q)
                wall["query"] += time.perf_counter() - t0
            outs.append(out)
        k = kernels(SPLIT_KERNELS if kind == "A" else STEP_KERNELS)
        ctx.timing(0)
        rec = {"kind": kind, "wall_ms_per_batch": {x: round(v * 1e3 / R, 4) for x, v in wall.items() if v},
               "kernel_ms_per_batch": k, "kernel_ms_sum": round(sum(k.values()), 4)}
        if kind == "A":
            rec["sets_per_batch"] = sets / R
            rec["wall_ms_round"] = round(sum(wall.values()) * 1e3 / R, 4)
        return rec, outs

    # every block's ids go to both twins, so their states stay equal: A B B A over pairs of id blocks
    warm = rng.integers(0, N, size=(2, NIDS), dtype=np.uint64)
    block("A", warm)
    block("B", warm)
    blocks = []
    for pair in range(2):
        ids = rng.integers(0, N, size=(R, NIDS), dtype=np.uint64)
        order = "AB" if pair == 0 else "BA"
        got = {}
        for kind in order:
            rec, got[kind] = block(kind, ids)
            blocks.append(rec)
            print(f"[probe] {rec}", file=sys.stderr, flush=True)
        assert all(np.array_equal(x, y) for x, y in zip(got["A"], got["B"])), pair
    A = [x for x in blocks if x["kind"] == "A"]
    B = [x for x in blocks if x["kind"] == "B"]
    round_ms = float(np.mean([x["wall_ms_round"] for x in A]))
    query_ms = float(np.mean([x["wall_ms_per_batch"]["query"] for x in B]))
    ss = cfg["SetSize"]
    print(json.dumps({"partitions": P, "rows": ROWS, "E": E, "n": NIDS, "batches_per_block": R, "blocks": blocks,
                      "split_round_wall_ms": round(round_ms, 4), "query_wall_ms": round(query_ms, 4),
                      "round_over_query": round(round_ms / query_ms, 2),
                      "bytes_down_per_full_batch": NIDS * ss * 4, "bytes_up_per_full_batch": NIDS * E * 8}))


if __name__ == "__main__":
    main()

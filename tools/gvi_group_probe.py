"""gvi_group_probe.py — host wall time per round of a server that keeps its own
beam search and fetches through the GetGraphInfo plugin surface:

  A  one pm_graph_group_get_vertex_info call per round for all sessions;
  B  the loop of one pm_graph_get_vertex_info call per session (the baseline);
  C  pm_search_loop_batched's time per round for the same sessions (the ceiling:
     the library's own loop, search included).

The shape is bench.py's SIFT1M-shaped graph and session count; every round
fetches parallel x m ids per session, recorded from a non-private beam search
of the session's own query over the same graph (so the ids repeat and cluster
as a search's do).  A and B run in one process on the same sessions, ordered
A B B A, three times; every block's figure is printed, then one JSON line.

    python tools/gvi_group_probe.py [--sessions 288] [--rounds 20] [--graph built|random]
"""
import argparse
import heapq
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def record_rounds(v, g, q, rounds, parallel, rng):
    """The ids of `rounds` rounds of a beam search for q (graphann/search.go:150-172): each round pops the
    `parallel` nearest unexpanded vertices and fetches their neighbour lists."""
    n, m = g.shape
    start = rng.choice(n, size=int(np.sqrt(n)), replace=False)
    d = ((v[start] - q) ** 2).sum(axis=1)
    heap = [(float(d[i]), int(start[i])) for i in np.argsort(d, kind="stable")[:parallel]]
    heapq.heapify(heap)
    known = {x for _, x in heap}
    out = []
    for _ in range(rounds):
        ids = []
        for _ in range(parallel):
            ids.extend(g[heapq.heappop(heap)[1]] if heap else rng.integers(0, n, size=m))
        ids = np.asarray(ids, dtype=np.uint64)
        out.append(ids)
        new = [int(x) for x in dict.fromkeys(ids.tolist()) if x not in known]
        if new:
            dn = ((v[new] - q) ** 2).sum(axis=1)
            for x, dx in zip(new, dn):
                known.add(x)
                heapq.heappush(heap, (float(dx), x))
    return out


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=bench.SESSIONS)
    ap.add_argument("--rounds", type=int, default=bench.STEP, help="rounds per block")
    ap.add_argument("--graph", choices=["built", "random"], default="built")
    args = ap.parse_args()
    import pacmann_amd as pm
    S, R, PAR = args.sessions, args.rounds, bench.PARALLEL
    ctx0 = pm.Context(0)
    v, g, _ = bench.make_data(0, args.graph, ctx0)
    dim = v.shape[1]
    blocks = "ABBA" * 3
    queries = bench.make_queries(v, S * (len(blocks) + 2), seed=900).reshape(S, len(blocks) + 2, dim)
    base = pm.PIRGraphInfo(v, g, pir_seed=11, search_seed=12, ctx=ctx0)
    base.Preprocess()
    sess = [base] + [base.Session(11 + i, 12 + i, pm.Context(0)) for i in range(1, S)]
    for s in sess[1:]:
        s.Preprocess()
    grp = pm.PIRGraphGroup(sess)
    rng = np.random.default_rng(901)
    print(f"[probe] {S} sessions ready; recording {len(blocks) + 1} x {R} rounds", file=sys.stderr, flush=True)
    rec = [[record_rounds(v, g, queries[s, b], R, PAR, rng) for s in range(S)] for b in range(len(blocks) + 1)]

    def run_a(b):
        t = 0.0
        for r in range(R):
            ids = [rec[b][s][r] for s in range(S)]
            t0 = time.perf_counter()
            grp.get_vertex_info(ids, queries[:, b])
            t += time.perf_counter() - t0
        return t / R

    def run_b(b):
        t = 0.0
        for r in range(R):
            t0 = time.perf_counter()
            for s in range(S):
                sess[s].GetVertexInfo(rec[b][s][r], queries[s, b])
            t += time.perf_counter() - t0
        return t / R
    run_a(len(blocks))   # warm-up: buffers, code objects
    prep0 = sum(s.PIR.stats()["PrepCount"] for s in sess)
    res = {"A": [], "B": []}
    for b, kind in enumerate(blocks):
        ms = (run_a if kind == "A" else run_b)(b) * 1e3
        res[kind].append(round(ms, 3))
        print(f"[probe] block {b} {kind}: {ms:.3f} ms per round", file=sys.stderr, flush=True)
    prep1 = sum(s.PIR.stats()["PrepCount"] for s in sess)
    steps = sess[0].ctx.timing_get("host_gvi_group_steps")[0]
    _, wall, _, mt = pm.search_loop_batched(sess, queries[:, -1:], bench.K_TOP, R, PAR, bench.GROUPS, bench.THREADS)
    out = {"sessions": S, "rounds_per_block": R, "ids_per_session_per_round": PAR * g.shape[1], "graph": args.graph,
           "A_group_ms_per_round": res["A"], "B_single_loop_ms_per_round": res["B"],
           "A_median": float(np.median(res["A"])), "B_median": float(np.median(res["B"])),
           "C_search_loop_batched_ms_per_round": round((wall - float(np.max(mt))) * 1e3 / R, 3),
           "re_preprocessings_in_blocks": prep1 - prep0, "group_shared_steps": steps}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""server_answer_probe.py — the batch PIR's server role (pm_batchpir_server_answer,
k_server_answer_parts) on the SIFT1M graph shape (n = 1M, dim 128, m 32: 16
partitions of 62,500 rows, 640-B entries, 384-B packed rows).

  1. Against the only comparable earlier code, pm_pir_server_answer
     (k_server_answer) on a lone pm_pir holding partition 0's rows (62,500 x 80
     words): the same offset sets go to A, the lone pm_pir ("answer" events);
     B, the graph server without the packed image, every set in partition 0
     ("server_answer" events); C, the same on the server with the packed image.
     Blocks run A B C C B A, three times, `--calls` calls each; the answers of
     the three must be equal.  The kernel time per call of every block is
     printed; the parent's spread is max - min over its six blocks.
  2. The call itself over all 16 partitions, packed and not, for several batch
     sizes: sets per second of wall time, wall time per call, and the kernel's
     gathered bytes per second (rows gathered x bytes read per row, over the
     events' time) as a fraction of the HBM peak.

One JSON line at the end.  Needs the GPU; about 2.5 GB of host memory.

    python tools/server_answer_probe.py [--sets 4096] [--calls 20]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N, DIM, M = 1_000_000, 128, 32
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4096, help="offset sets per call in part 1")
    ap.add_argument("--calls", type=int, default=20, help="calls per block")
    ap.add_argument("--n", type=int, default=N, help="vertices (the default is the shape the figures are for)")
    args = ap.parse_args()
    import pacmann_amd as pm
    n = args.n
    ctx = pm.Context(0)
    rng = np.random.default_rng(1)
    v = rng.integers(0, 256, size=(n, DIM)).astype(np.float32)   # bvecs semantics: packable
    g = rng.integers(0, n, size=(n, M), dtype=np.uint32)
    E = (DIM + M) // 2

    def graph_server(pack):
        pm.set_option("answer_pack", pack)
        gi = pm.PIRGraphInfo(v, g, skip_prep=True, pir_seed=5, search_seed=6, ctx=ctx)
        gi.Preprocess()   # makes the server; skip_prep: no hints are built, the role needs none
        return gi
    try:
        plain, packed = graph_server(0), graph_server(1)
    finally:
        pm.set_option("answer_pack", -1)
    pirs = {"B": plain.PIR, "C": packed.PIR}
    cfgs = [pirs["B"].SubConfig(p) for p in range(pirs["B"].Config()["PartitionNum"])]
    c0 = cfgs[0]
    raw0 = np.concatenate([v[:c0["DBSize"]].view(np.uint32), g[:c0["DBSize"]]], axis=1).copy().view(np.uint64).ravel()
    lone = pm.PianoPIR(c0["DBSize"], E * 8, raw0, 8, seed=5, ctx=ctx)
    assert lone.Config()["SetSize"] == c0["SetSize"] and lone.Config()["ChunkSize"] == c0["ChunkSize"]
    ss, stride = c0["SetSize"], pirs["B"].max_set_size
    print(f"[probe] {len(cfgs)} partitions of {c0['DBSize']} rows, SetSize {ss}, ChunkSize {c0['ChunkSize']}",
          file=sys.stderr, flush=True)

    # ---- part 1: A B C C B A on partition 0's shape ----
    S, R = args.sets, args.calls
    offs = np.zeros((S, stride), dtype=np.uint32)
    offs[:, :ss] = rng.integers(0, c0["ChunkSize"], size=(S, ss), dtype=np.uint32)
    offs_lone = np.ascontiguousarray(offs[:, :ss])
    part0 = np.zeros(S, dtype=np.uint32)

    def block(kind):
        """(kernel ms per call, wall ms per call, gathered bytes per call) of R calls."""
        ctx.timing_reset()
        ctx.timing(1)
        t0 = time.perf_counter()
        for _ in range(R):
            if kind == "A":
                lone.PrivateQuery(offs_lone)
            else:
                pirs[kind].ServerAnswer(part0, offs)
        wall = (time.perf_counter() - t0) * 1e3 / R
        nl, ms, by = ctx.timing_get("answer" if kind == "A" else "server_answer")
        ctx.timing(0)
        assert nl == R, (kind, nl)
        return ms / R, wall, by / R
    want = lone.PrivateQuery(offs_lone)   # also the warm-up of every path
    for k in "BC":
        assert np.array_equal(pirs[k].ServerAnswer(part0, offs), want), k
    res = {k: [] for k in "ABC"}
    for b, kind in enumerate("ABCCBA" * 3):
        ms, wall, by = block(kind)
        res[kind].append({"kernel_ms": round(ms, 4), "wall_ms": round(wall, 3), "gathered_GBps": round(by / ms / 1e6, 1)})
        print(f"[probe] block {b} {kind}: kernel {ms:.4f} ms, wall {wall:.3f} ms per call of {S} sets",
              file=sys.stderr, flush=True)
    med = {k: float(np.median([x["kernel_ms"] for x in res[k]])) for k in "ABC"}
    a = [x["kernel_ms"] for x in res["A"]]
    part1 = {"sets_per_call": S, "calls_per_block": R, "blocks": res, "kernel_ms_median": med,
             "parent_spread_ms": round(max(a) - min(a), 4), "B_minus_A_ms": round(med["B"] - med["A"], 4),
             "B_within_parent_spread": bool(med["B"] - med["A"] <= max(a) - min(a)),
             "C_over_A": round(med["C"] / med["A"], 4), "C_over_B": round(med["C"] / med["B"], 4)}

    # ---- part 2: all partitions ----
    part2 = []
    for nq in (16, 256, 4096, 16384):
        parts = (np.arange(nq) % len(cfgs)).astype(np.uint32)
        o = np.zeros((nq, stride), dtype=np.uint32)
        for p, c in enumerate(cfgs):
            sel = np.where(parts == p)[0]
            o[sel, :c["SetSize"]] = rng.integers(0, c["ChunkSize"], size=(len(sel), c["SetSize"]), dtype=np.uint32)
        outs = {}
        for kind in "BCCB":
            pir = pirs[kind]
            pir.ServerAnswer(parts, o)   # warm-up at this size
            ctx.timing_reset()
            ctx.timing(1)
            t0 = time.perf_counter()
            for _ in range(R):
                out = pir.ServerAnswer(parts, o)
            wall = (time.perf_counter() - t0) / R
            nl, ms, by = ctx.timing_get("server_answer")
            ctx.timing(0)
            outs[kind] = out
            gbps = by / ms / 1e6
            part2.append({"answer_pack": int(kind == "C"), "sets": nq, "wall_ms_per_call": round(wall * 1e3, 3),
                          "sets_per_s": round(nq / wall), "kernel_ms_per_call": round(ms / nl, 4),
                          "gathered_GBps": round(gbps, 1), "fraction_of_hbm_peak": round(gbps / HBM_PEAK_GBS, 3)})
            print(f"[probe] {part2[-1]}", file=sys.stderr, flush=True)
        assert np.array_equal(outs["B"], outs["C"]), nq
    print(json.dumps({"n": n, "dim": DIM, "m": M, "vs_parent_partition0": part1, "all_partitions": part2}))


if __name__ == "__main__":
    main()

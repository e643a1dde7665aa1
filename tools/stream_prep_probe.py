"""stream_prep_probe.py — the streamed hint preprocessing (pm_batchpir_prep_stream_*)
on SIFT1M's batch-PIR shape: 16 partitions x 62,500 rows x 80 words, 640 MB of
rows per stream.

A server handle, a client twin of it (its Preprocessing() is the whole-DB
figure) and a remote handle with no DB, streamed from the host copy of the rows
(so that only the client's side is timed).  For each window size (one chunk, 8
chunks, a whole partition per call), after one warm-up stream, blocks run
A B B A of `--streams` streams each: A is the stream as it is, B the
upload-only pass (pm_set_option "stream_upload_only": the same sub-windows
through the same staging, the two kernels not launched).  Wall time per stream
is begin to end inclusive.  One more stream per window size runs with timing
level 1 for the kernel time of k_stream_fold / k_stream_repl (its wall time is
not used: every launch carries two events).  The quantity to judge is
streamed wall time over upload-only wall time of the same run.  At the end a
real stream must equal the twin.  One JSON line, also written to --out.  Needs
the GPU; about 2 GB of host memory.

    timeout -k 10 300 python tools/stream_prep_probe.py [--streams 3] [--out FILE]

(under a time limit, as every GPU step: the probe sets none itself)
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

P, ROWS, E, F = 16, 62_500, 80, 8
KERNELS = ("prep_stream_fold", "prep_stream_repl")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=3, help="streams per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pacmann_amd as pm
    ctx = pm.Context(0)
    N = P * ROWS
    db = np.random.default_rng(1).integers(0, 2**64, size=N * E, dtype=np.uint64)
    rows = db.reshape(N, E)
    server = pm.SimpleBatchPianoPIR(N, E * 8, 2 * P, db, F, seed=11, ctx=ctx)
    twin = server.Client(5)
    remote = pm.SimpleBatchPianoPIR.Remote(N, E * 8, 2 * P, F, seed=5, ctx=ctx)
    cfg = remote.SubConfig(0)
    cs, ss = cfg["ChunkSize"], cfg["SetSize"]
    print(f"[probe] {P} partitions of {cfg['DBSize']} rows, SetSize {ss}, ChunkSize {cs}, "
          f"hints {cfg['PrimaryHintNum'] + ss * cfg['MaxQueryPerChunk']}", file=sys.stderr, flush=True)

    def windows(per):
        return [(p, c0, min(per, ss - c0)) for p in range(P) for c0 in range(0, ss, per)]

    def one_stream(wins):
        t0 = time.perf_counter()
        remote.PrepStreamBegin()
        for p, c0, nc in wins:
            remote.PrepStreamRows(p, c0, nc, rows[p * ROWS + c0 * cs: p * ROWS + min((c0 + nc) * cs, ROWS)])
        remote.PrepStreamEnd()
        return (time.perf_counter() - t0) * 1e3

    twin_ms = []
    for _ in range(1 + args.streams):
        t0 = time.perf_counter()
        twin.Preprocessing()
        twin_ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    result = {"partitions": P, "rows": ROWS, "E": E, "F": F, "ChunkSize": cs, "SetSize": ss,
              "upload_bytes_per_stream": N * E * 8, "streams_per_block": args.streams,
              "twin_preprocessing_ms": twin_ms[1:], "window_sizes": {}}
    for label, per in (("1 chunk", 1), ("8 chunks", 8), ("whole partition", ss)):
        wins = windows(per)
        one_stream(wins)   # warm-up (the first one also allocates the staging slots)
        blocks = []
        for kind in "ABBA":
            pm.set_option("stream_upload_only", 1 if kind == "B" else 0)
            ctx.timing_reset()
            ms = [round(one_stream(wins), 3) for _ in range(args.streams)]
            subw = ctx.timing_get("host_prep_stream_windows")[0] // args.streams
            blocks.append({"kind": "stream" if kind == "A" else "upload_only", "wall_ms": ms, "sub_windows": subw})
            print(f"[probe] {label}: {blocks[-1]}", file=sys.stderr, flush=True)
        pm.set_option("stream_upload_only", 0)
        ctx.timing_reset()
        ctx.timing(1)
        one_stream(wins)
        kern = {k: {"launches": ctx.timing_get(k)[0], "ms": round(ctx.timing_get(k)[1], 3)} for k in KERNELS}
        ctx.timing(0)
        a = float(np.mean([x for b in blocks if b["kind"] == "stream" for x in b["wall_ms"]]))
        u = float(np.mean([x for b in blocks if b["kind"] == "upload_only" for x in b["wall_ms"]]))
        result["window_sizes"][label] = {"calls": len(wins), "blocks": blocks, "kernel_ms_per_stream": kern,
                                         "stream_wall_ms": round(a, 3), "upload_only_wall_ms": round(u, 3),
                                         "stream_over_upload_only": round(a / u, 3)}
    # the probe's streams are real ones: the last epoch equals the twin's
    epochs = 3 * (1 + 4 * args.streams + 1)
    for _ in range(epochs + 1 - len(twin_ms)):
        twin.Preprocessing()
    one_stream(windows(ss))
    a, b = remote.export_state(3), twin.export_state(3)
    result["equals_twin"] = all(np.array_equal(a[k], b[k]) for k in a)
    assert result["equals_twin"]
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()

"""Usage: [PM_LIB=<another build of the library>] python profiles/step_spec/step_perf_one.py <label>
One process: the one-client TestBatchPIRPerf shape (configs[2]) through k_step, uninstrumented; one JSON line."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "..")))
import pacmann_amd as pm
N, E, B, NB = 3_201_821, 112, 32, 300
ctx = pm.default_context()
db = np.random.default_rng(77).integers(0, 2**64, size=N * E, dtype=np.uint64)
g = pm.SimpleBatchPianoPIR(N, E * 8, B, db, 8, seed=21, ctx=ctx)
g.Preprocessing()
batches = np.random.default_rng(78).integers(0, N, size=(5 * NB + 10, B)).astype(np.uint64)
for b in batches[:10]:
    g.Query(b)
ctx.sync()
out = []
for k in range(4):   # the first pass is discarded (below): it still holds start-up effects
    t0 = time.perf_counter()
    for b in batches[10 + k * NB:10 + (k + 1) * NB]:
        g.Query(b)
    ctx.sync()
    out.append(round((time.perf_counter() - t0) / NB * 1e6, 2))
# k_step's own time: a further pass with the kernel's events on (as bench.py's kernel_timing_pass)
ctx.timing_reset()
ctx.timing(2)
for b in batches[10 + 4 * NB:]:
    g.Query(b)
ctx.sync()
ctx.timing(False)
n, ms, _ = ctx.timing_get("step")
print(json.dumps({"lib": sys.argv[1], "us_per_batch": out[1:], "discarded_first_pass": out[0],
                  "k_step_us": round(ms / n * 1e3, 3), "k_step_launches": n}), flush=True)

"""Streamed hint preprocessing (pm_batchpir_create_remote, pm_batchpir_prep_stream_begin / _rows / _end,
pm_batchpir_prep_due, pm_batchpir_server_rows).

Three handles over one DB: a server that is never preprocessed, a Client(seed) twin preprocessed with
Preprocessing(), and a Remote(seed) handle with no DB whose hints come from the server's rows, window by window.
After a completed stream the remote equals the twin bit for bit in every partition's exported state and in the
counters, and both equal the oracle's SimpleBatchPianoPIR.  Every comparison is exact (XORs, indices).
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import SEED, STATE_KEYS
from tests.test_gpu_split_query import GRAPH, PM_EINVAL, assert_same, graph_inputs, raw_begin, raw_finish, snapshot

pytestmark = pytest.mark.gpu

STREAM_OPEN = "a streamed preprocessing is open"
NO_DB = "no DB on this handle"
DUE = "preprocessing due: stream it first"

# name -> N, E (words), BatchSize, F.  What each is chosen for is asserted in shape_facts.
SHAPES = {
    "A": dict(N=4 * 2500, E=8, B=8, F=4),      # the last chunk is partial
    "B": dict(N=GRAPH["N"], E=GRAPH["E"], B=GRAPH["B"], F=GRAPH["F"]),   # the graph entry; partitions of different length
    "C": dict(N=2 * 2100, E=8, B=4, F=4),      # chunks 17-19 wholly past the end, chunk 16 partial
    "D": dict(N=2 * 1500, E=5, B=4, F=4),      # odd E: W = 1
    "E": dict(N=2 * 1500, E=3, B=4, F=4),      # E < 4: the xor is empty, only ridx / rval move
    "F": dict(N=2 * 20000, E=8, B=4, F=4),     # ChunkSize 512
    "G": dict(N=2 * 20000, E=80, B=4, F=4),    # a partition above 8 MiB: the sub-window split
}
_dbs = {}


def shape_db(name):
    """The shape's DB, built once and read-only (B's is graph_inputs')."""
    assert name != "B"
    if name not in _dbs:
        s = SHAPES[name]
        _dbs[name] =np.random.default_rng(sum(map(ord, name)) + 700).integers(0, 2**64, size=s["N"] * s["E"], dtype=np.uint64)
    return _dbs[name]


def make(ctx, name, db, seed=SEED, with_remote=True):
    """(server never preprocessed, twin client not yet preprocessed, remote, per-partition SubConfigs)."""
    import pacmann_amd as pm
    s = SHAPES[name]
    server = pm.SimpleBatchPianoPIR(s["N"], s["E"] * 8, s["B"], db, s["F"], seed=seed + 999, ctx=ctx)
    twin = server.Client(seed)
    remote = pm.SimpleBatchPianoPIR.Remote(s["N"], s["E"] * 8, s["B"], s["F"], seed=seed, ctx=ctx) if with_remote else None
    P = server.Config()["PartitionNum"]
    cfgs = [server.SubConfig(p) for p in range(P)]
    return server, twin, remote, cfgs


def shape_facts(name, cfgs):
    """The property each shape is chosen for, from the handles' own SubConfig."""
    cs, ss, n = [c["ChunkSize"] for c in cfgs], [c["SetSize"] for c in cfgs], [c["DBSize"] for c in cfgs]
    for c in cfgs:
        assert c["SetSize"] % 4 == 0 and (c["SetSize"] - 4) * c["ChunkSize"] < c["DBSize"] <= c["SetSize"] * c["ChunkSize"]
    if name == "A":
        assert len(cfgs) == 4 and n == [2500] * 4
        assert all(x % c != 0 and (s - 1) * c < x for x, c, s in zip(n, cs, ss))   # the last chunk is partial
    if name == "B":
        assert len(set(n)) > 1 and cfgs[0]["DBEntrySize"] == 80
    if name == "C":
        assert cs == [128, 128] and ss == [20, 20] and n == [2100, 2100]
        assert 16 * 128 < 2100 < 17 * 128   # chunk 16 partial, 17-19 wholly past the end
    if name == "D":
        assert cfgs[0]["DBEntrySize"] == 5
    if name == "E":
        assert cfgs[0]["DBEntrySize"] == 3
    if name == "F":
        assert cs == [512, 512]
    if name == "G":
        assert cfgs[0]["DBEntrySize"] == 80 and n[0] * 640 > (8 << 20)
        assert ss[0] * cs[0] * 640 > (8 << 20) >= cs[0] * 640


def part_rows(db, s, cfgs, p, c0, nc):
    """Rows of chunks [c0, c0 + nc) of partition p, from the numpy DB."""
    P = len(cfgs)
    PS = (s["N"] + P - 1) // P
    rows = db.reshape(s["N"], s["E"])[p * PS: p * PS + cfgs[p]["DBSize"]]
    return rows[c0 * cfgs[p]["ChunkSize"]: (c0 + nc) * cfgs[p]["ChunkSize"]]


def stream(h, windows, rows_of):
    """One whole stream of `windows` [(partition, chunk0, nchunks)]."""
    h.PrepStreamBegin()
    for p, c0, nc in windows:
        h.PrepStreamRows(p, c0, nc, rows_of(p, c0, nc))
    h.PrepStreamEnd()


def whole(cfgs):
    return [(p, 0, c["SetSize"]) for p, c in enumerate(cfgs)]


def straddling(cfgs):
    """Windows that straddle tabT's 8-chunk tiles: (3, 5), (8, 1), (9, 11) among them."""
    out = []
    for p, c in enumerate(cfgs):
        ss = c["SetSize"]
        assert ss >= 20
        out += [(p, 0, 3), (p, 3, 5), (p, 8, 1), (p, 9, 11)] + ([(p, 20, ss - 20)] if ss > 20 else [])
    return out


def oracle_state(oracle, name, db):
    s = SHAPES[name]
    o = oracle.SimpleBatchPianoPIR(s["N"], s["E"] * 8, s["B"], db, s["F"], seed=SEED)
    o.Preprocessing()
    return [o.sub(p).export_state() for p in range(o.stats()["PartitionNum"])], o.stats()


# ---------------------------------------------------------------------------
# 1. twin equality and the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E", "F"])
def test_twin_and_oracle(ctx, oracle, name):
    ref = graph_inputs(oracle) if name == "B" else None
    db = ref["db"] if ref else shape_db(name)
    server, twin, remote, cfgs = make(ctx, name, db)
    shape_facts(name, cfgs)
    P = len(cfgs)
    twin.Preprocessing()
    remote.StreamPreprocessingFrom(server)
    assert not remote.prep_due
    assert_same(snapshot(remote, P), snapshot(twin, P), name)
    ostate, ostats = oracle_state(oracle, name, db)
    for p in range(P):
        got = remote.export_state(p)
        for k in STATE_KEYS:
            assert np.array_equal(got[k], ostate[p][k]), (name, p, k)
    for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
        assert remote.stats()[key] == ostats[key], key
    if name == "E":   # nothing was folded: the parities are zero, the replacement rows are not
        assert not remote.export_state(0)["primary_parity"].any() and remote.export_state(0)["repl_val"].any()
    if name == "C":   # the chunks past the end have their indices and zero values
        st, c = remote.export_state(0), cfgs[0]
        q, e = c["MaxQueryPerChunk"], c["DBEntrySize"]
        assert (st["repl_idx"][17 * q:] >= 17 * 128).all() and (st["repl_idx"][17 * q:] < 20 * 128).all()
        assert not st["repl_val"][17 * q * e:].any()


# ---------------------------------------------------------------------------
# 2. window geometry; the sub-window split
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
def test_window_geometry(ctx, oracle, name):
    import pacmann_amd as pm
    s = SHAPES[name]
    db = graph_inputs(oracle)["db"] if name == "B" else shape_db(name)
    server, twin, _, cfgs = make(ctx, name, db, with_remote=False)
    P = len(cfgs)
    twin.Preprocessing()
    want = snapshot(twin, P)
    shuffled = straddling(cfgs)
    np.random.default_rng(5).shuffle(shuffled)
    geoms = {
        "one chunk per call": [(p, c, 1) for p, cf in enumerate(cfgs) for c in range(cf["SetSize"])],
        "whole partitions": whole(cfgs),
        "straddling": straddling(cfgs),
        "shuffled": [tuple(int(x) for x in w) for w in shuffled],
    }
    assert geoms["shuffled"] != geoms["straddling"] and sorted(geoms["shuffled"]) == sorted(geoms["straddling"])
    for what, windows in geoms.items():
        r = pm.SimpleBatchPianoPIR.Remote(s["N"], s["E"] * 8, s["B"], s["F"], seed=SEED, ctx=ctx)
        stream(r, windows, lambda p, c0, nc: part_rows(db, s, cfgs, p, c0, nc))
        assert_same(snapshot(r, P), want, (name, what))


def test_sub_window_split(ctx):
    """A call larger than 8 MiB is cut into sub-windows of whole chunks that alternate between the two
    staging slots; the kernels are launched once per sub-window."""
    name = "G"
    db = shape_db(name)
    server, twin, remote, cfgs = make(ctx, name, db)
    shape_facts(name, cfgs)
    P = len(cfgs)
    twin.Preprocessing()
    ctx.timing_reset()
    ctx.timing(1)
    try:
        remote.StreamPreprocessingFrom(server)   # whole partitions: P calls
        folds, repls = ctx.timing_get("prep_stream_fold")[0], ctx.timing_get("prep_stream_repl")[0]
    finally:
        ctx.timing(0)
    windows = ctx.timing_get("host_prep_stream_windows")[0]
    per = (8 << 20) // (cfgs[0]["ChunkSize"] * 640)
    assert windows == sum(-(-c["SetSize"] // per) for c in cfgs) and windows > P
    assert folds == windows and repls == windows
    assert ctx.timing_get("host_prep_stream")[0] == 1
    assert_same(snapshot(remote, P), snapshot(twin, P), name)


# ---------------------------------------------------------------------------
# 3. second epoch; begin on an open stream
# ---------------------------------------------------------------------------
def test_epochs_and_abandoned_stream(ctx):
    """Every begin takes the next epoch's keys, a completed stream counts one preprocessing.  So two streams
    equal two Preprocessing calls, and a handle that streamed once, lost its second stream half way (a dropped
    connection) and began again has the hints of a twin after three preprocessings, its own PrepCount being 2:
    the abandoned stream cost an epoch."""
    import pacmann_amd as pm
    name = "A"
    s = SHAPES[name]
    db = shape_db(name)
    server, twin, remote, cfgs = make(ctx, name, db)
    P = len(cfgs)
    for _ in range(2):
        twin.Preprocessing()
        remote.StreamPreprocessingFrom(server, chunks_per_window=7)
    assert remote.stats()["PrepCount"] == 2
    assert_same(snapshot(remote, P), snapshot(twin, P), "two epochs")
    lossy = pm.SimpleBatchPianoPIR.Remote(s["N"], s["E"] * 8, s["B"], s["F"], seed=SEED, ctx=ctx)
    lossy.StreamPreprocessingFrom(server)
    lossy.PrepStreamBegin()
    lossy.PrepStreamRows(1, 0, 9, server.ServerRows(1, 0, 9))
    lossy.StreamPreprocessingFrom(server)   # its begin finds the stream open
    twin.Preprocessing()
    got, want = snapshot(lossy, P), snapshot(twin, P)
    assert (got[0].pop("PrepCount"), want[0].pop("PrepCount")) == (2, 3)
    assert_same(got, want, "after an abandoned stream")


# ---------------------------------------------------------------------------
# 4. online after streaming
# ---------------------------------------------------------------------------
def test_online_after_streaming(ctx, oracle):
    ref = graph_inputs(oracle)
    server, twin, remote, cfgs = make(ctx, "B", ref["db"])
    P = len(cfgs)
    twin.Preprocessing()
    remote.StreamPreprocessingFrom(server, chunks_per_window=6)
    for b in range(GRAPH["batches"]):
        parts, offs = remote.QueryBegin(ref["ids"][b])
        out, ok = remote.QueryFinish(server.ServerAnswer(parts, offs))
        outb, okb = twin.QueryWithMask(ref["ids"][b])
        assert np.array_equal(out, outb) and np.array_equal(ok, okb) and np.array_equal(out, ref["want"][b]), b
        assert_same(snapshot(remote, P), snapshot(twin, P), b)


# ---------------------------------------------------------------------------
# 5. across the trigger
# ---------------------------------------------------------------------------
def test_across_the_trigger(ctx):
    name = "A"
    db = shape_db(name)
    server, twin, remote, cfgs = make(ctx, name, db)
    P, rows = len(cfgs), 2500
    twin.Preprocessing()
    remote.StreamPreprocessingFrom(server)
    rng = np.random.default_rng(66)
    maxq = remote.SubConfig(0)["MaxQueryNum"]

    def batch():
        q = (np.arange(P) * rows + rng.integers(0, rows, size=P)).astype(np.uint64)   # one id per partition
        parts, offs = remote.QueryBegin(q)
        out, ok = remote.QueryFinish(server.ServerAnswer(parts, offs))
        outb, okb = twin.QueryWithMask(q)
        assert np.array_equal(out, outb) and np.array_equal(ok, okb)
        return q

    batches = 0
    while twin.stats()["PrepCount"] < 2:
        assert batches <= maxq + 8 and not remote.prep_due   # the trigger fires by MaxQueryNum - 2 batches
        if batches % 64 == 0:
            assert_same(snapshot(remote, P), snapshot(twin, P), batches)
        q = batch()
        batches += 1
    assert batches > 5 and remote.prep_due and remote.stats()["PrepCount"] == 1
    before = snapshot(remote, P)
    rc, msg, _, _ = raw_begin(remote, q)
    assert rc == PM_EINVAL and DUE in msg, (rc, msg)
    assert_same(snapshot(remote, P), before, "refused begin")
    assert remote.prep_due
    remote.StreamPreprocessingFrom(server, chunks_per_window=8)
    assert not remote.prep_due and remote.stats()["PrepCount"] == 2
    assert_same(snapshot(remote, P), snapshot(twin, P), "after the stream")
    for i in range(4):
        batch()
        assert_same(snapshot(remote, P), snapshot(twin, P), ("after", i))


# ---------------------------------------------------------------------------
# 6. a handle with a DB
# ---------------------------------------------------------------------------
def test_handle_with_a_db(ctx):
    name = "F"
    db = shape_db(name)
    server, twin, _, cfgs = make(ctx, name, db, with_remote=False)
    P = len(cfgs)
    other = server.Client(SEED)
    twin.Preprocessing()
    other.StreamPreprocessingFrom(server, chunks_per_window=5)
    assert_same(snapshot(other, P), snapshot(twin, P), "client streamed from its server")
    # ... and it is an ordinary client afterwards
    q = np.array([3, 20000 + 5, 77, 20000 + 9], dtype=np.uint64)
    out, ok = other.QueryWithMask(q)
    outb, okb = twin.QueryWithMask(q)
    assert np.array_equal(out, outb) and np.array_equal(ok, okb)
    assert_same(snapshot(other, P), snapshot(twin, P), "after a query")


# ---------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------
def raw_rows(pir, p, c0, nc, rows, nrows):
    import pacmann_amd as pm
    ptr = None if rows is None else np.ascontiguousarray(rows, dtype=np.uint64).ctypes.data_as(pm.u64p)
    rc = pm.lib().pm_batchpir_prep_stream_rows(pir.h, p, c0, nc, ptr, nrows)
    return rc, pm.lib().pm_last_error().decode()


def wrapped(fn):   # a Python wrapper's RuntimeError as (code, message)
    try:
        fn()
    except RuntimeError as e:
        return PM_EINVAL if f"error {PM_EINVAL}:" in str(e) else 0, str(e)
    return 0, ""


def test_refusals(ctx):
    import pacmann_amd as pm
    name = "A"
    s = SHAPES[name]
    db = shape_db(name)
    server, twin, remote, cfgs = make(ctx, name, db)
    P, E = len(cfgs), s["E"]
    cs, ss = cfgs[0]["ChunkSize"], cfgs[0]["SetSize"]
    other = server.Client(SEED + 5)
    other.Preprocessing()
    q = (np.arange(P) * 2500 + 7).astype(np.uint64)

    def refused(call, text, handles=(remote,)):
        before = [snapshot(h, P) for h in handles]
        rc, msg = call()
        assert rc == PM_EINVAL and text in msg, (text, rc, msg)
        for h, b in zip(handles, before):
            assert_same(snapshot(h, P), b, text)

    full = np.zeros((cs, E), dtype=np.uint64)
    # no stream yet
    refused(lambda: raw_rows(remote, 0, 0, 1, full, cs), "no streamed preprocessing is open")
    refused(lambda: wrapped(remote.PrepStreamEnd), "no streamed preprocessing is open")
    refused(lambda: raw_begin(remote, q)[:2], "not preprocessed")
    # every "no DB on this handle" call
    refused(lambda: wrapped(lambda: remote.Query(q)), NO_DB)
    refused(lambda: wrapped(lambda: remote.QueryWithMask(q)), NO_DB)
    refused(lambda: wrapped(remote.Preprocessing), NO_DB)
    refused(lambda: wrapped(lambda: remote.ServerAnswer(np.zeros(1, np.uint32), np.zeros((1, ss), np.uint32))), NO_DB)
    refused(lambda: wrapped(lambda: remote.ServerRows(0, 0, 1)), NO_DB)
    refused(lambda: wrapped(lambda: remote.Client(3)), NO_DB)
    refused(lambda: wrapped(lambda: pm.BatchPIRGroup([other, remote])), NO_DB, (remote, other))
    refused(lambda: wrapped(lambda: pm.BatchPIRGroup([remote, other])), NO_DB, (remote, other))
    # an open stream: the rows rules
    remote.PrepStreamBegin()
    remote.PrepStreamRows(2, 4, 3, server.ServerRows(2, 4, 3))
    refused(lambda: raw_rows(remote, P, 0, 1, full, cs), "partition out of range")
    refused(lambda: raw_rows(remote, 0, 0, 0, full, 0), "nchunks")
    refused(lambda: raw_rows(remote, 0, ss - 1, 2, full, cs), "SetSize")
    refused(lambda: raw_rows(remote, 0, ss, 1, full, cs), "SetSize")
    refused(lambda: raw_rows(remote, 0, 0, 1, full, cs - 1), "nrows must be")
    refused(lambda: raw_rows(remote, 0, ss - 1, 1, full, cs), "nrows must be")   # the partial last chunk
    refused(lambda: raw_rows(remote, 0, 0, 1, None, cs), "rows is NULL")
    for c0, nc in ((4, 1), (6, 1), (3, 2), (6, 2), (0, ss)):
        refused(lambda: raw_rows(remote, 2, c0, nc, np.zeros((nc * cs, E)), min((c0 + nc) * cs, 2500) - c0 * cs),
                "chunk already delivered")
    # client calls while it is open
    refused(lambda: raw_begin(remote, q)[:2], STREAM_OPEN)
    refused(lambda: raw_finish(remote, np.zeros((1, E)), 1, P)[:2], STREAM_OPEN)
    refused(lambda: wrapped(remote.DummyPreprocessing), STREAM_OPEN)
    # end with one chunk missing names it; the stream stays open and completes
    for p, c0, nc in [w for w in straddling(cfgs) if w[0] != 2] + [(2, 0, 4), (2, 7, 4), (2, 12, 8)]:
        remote.PrepStreamRows(p, c0, nc, server.ServerRows(p, c0, nc))
    refused(lambda: wrapped(remote.PrepStreamEnd), "chunks missing: partition 2, chunk 11")
    remote.PrepStreamRows(2, 11, 1, server.ServerRows(2, 11, 1))
    remote.PrepStreamEnd()
    twin.Preprocessing()
    assert_same(snapshot(remote, P), snapshot(twin, P), "the stream was as it was")
    # a client with a DB while its stream is open: queries and group calls
    grp = pm.BatchPIRGroup([twin, other])
    twin.PrepStreamBegin()
    both = (twin, other)
    refused(lambda: wrapped(lambda: twin.Query(q)), STREAM_OPEN, both)
    refused(lambda: wrapped(lambda: twin.QueryWithMask(q)), STREAM_OPEN, both)
    refused(lambda: wrapped(lambda: grp.QueryWithMask(np.stack([q, q]))), STREAM_OPEN, both)
    refused(lambda: wrapped(grp.Preprocessing), STREAM_OPEN, both)
    twin.Preprocessing()   # allowed on a handle with a DB: it abandons the stream
    refused(lambda: wrapped(twin.PrepStreamEnd), "no streamed preprocessing is open", both)
    # a shard handle
    sh = pm.SimpleBatchPianoPIR(s["N"], E * 8, s["B"], db, s["F"], seed=SEED, ctx=ctx, shard=0, nshards=2)
    rc, msg = wrapped(sh.PrepStreamBegin)
    assert rc == PM_EINVAL and "shard handles" in msg, msg
    rc, msg = raw_rows(sh, 0, 0, 1, full, cs)
    assert rc == PM_EINVAL and "no streamed preprocessing is open" in msg, msg


# ---------------------------------------------------------------------------
# 8. ServerRows
# ---------------------------------------------------------------------------
def test_server_rows(ctx):
    import pacmann_amd as pm
    name = "C"
    s = SHAPES[name]
    db = shape_db(name)
    server, twin, _, cfgs = make(ctx, name, db, with_remote=False)
    P = len(cfgs)
    twin.Preprocessing()
    fresh = server.Client(SEED + 1)   # a client handle that was never preprocessed
    before = snapshot(twin, P)
    ranges = [(0, 20), (0, 1), (5, 9), (15, 2), (16, 1), (16, 4), (17, 1), (17, 3), (19, 1)]   # full, partial, past the end
    for h in (server, twin, fresh):
        for p in range(P):
            for c0, nc in ranges:
                got = h.ServerRows(p, c0, nc)
                want = part_rows(db, s, cfgs, p, c0, nc)
                assert got.shape == want.shape and np.array_equal(got, want), (p, c0, nc)
    assert server.ServerRows(1, 17, 3).shape == (0, s["E"]) and server.ServerRows(0, 16, 1).shape == (2100 - 2048, s["E"])
    # cap_rows too small: refused with *nrows set and nothing written
    buf = np.full((128, s["E"]), 0xA5A5, dtype=np.uint64)
    n = C.c_uint64(0)
    rc = pm.lib().pm_batchpir_server_rows(twin.h, 1, 3, 1, buf.ctypes.data_as(pm.u64p), 127, C.byref(n))
    assert rc == PM_EINVAL and "cap_rows" in pm.lib().pm_last_error().decode() and n.value == 128
    assert (buf == 0xA5A5).all()
    rc = pm.lib().pm_batchpir_server_rows(twin.h, 1, 3, 1, buf.ctypes.data_as(pm.u64p), 128, C.byref(n))
    assert rc == 0 and n.value == 128 and np.array_equal(buf, part_rows(db, s, cfgs, 1, 3, 1))
    for args, text in (((P, 0, 1), "partition out of range"), ((0, 0, 0), "nchunks"), ((0, 19, 2), "SetSize")):
        rc = pm.lib().pm_batchpir_server_rows(twin.h, *args, buf.ctypes.data_as(pm.u64p), 128, C.byref(n))
        assert rc == PM_EINVAL and text in pm.lib().pm_last_error().decode(), args
    assert_same(snapshot(twin, P), before, "client state untouched")

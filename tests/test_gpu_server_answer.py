"""pm_batchpir_server_answer: the batch PIR's server role for remote clients.

A client that keeps its keys and hints elsewhere sends, per query, a partition
and that partition's SetSize offsets; the server returns
PianoPIRServer.PrivateQuery (pir.go:65-88) of the set over the partition's
slice of the DB.  The checker below restates those lines in numpy over the
test's own rawDB, with each partition's DBSize / ChunkSize / SetSize from
pm_batchpir_subconfig and row0 = the sum of the earlier partitions' DBSize.
Every comparison is bit-exact.

The handles are not preprocessed unless the test is about client state: the
call reads the DB only.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20241021
PM_EINVAL = -1


def rand_db(n, e, seed):
    return np.random.default_rng(seed).integers(0, 2**64, size=n * e, dtype=np.uint64)


def subconfigs(pir):
    return [pir.SubConfig(p) for p in range(pir.Config()["PartitionNum"])]


def in_range(cfgs, parts, offs):
    """[nq, stride] bool: the terms pir.go:75-77 keeps (False past SetSize too)."""
    keep = np.zeros(offs.shape, dtype=bool)
    for p, c in enumerate(cfgs):
        sel = np.where(parts == p)[0]
        ss = c["SetSize"]
        r = np.arange(ss, dtype=np.uint64)[None, :] * np.uint64(c["ChunkSize"]) + offs[sel, :ss]
        keep[sel[:, None], np.arange(ss)[None, :]] = r < c["DBSize"]
    return keep


def private_query(raw, E, cfgs, parts, offs):
    """pir.go:65-88 for every set: XOR of the rows i*ChunkSize + offsets[i] < DBSize
    of the set's partition, over words [0, E & ~3) (EntryXor); the rest zero."""
    db = np.asarray(raw, dtype=np.uint64).reshape(-1, E)
    parts = np.asarray(parts)
    EX = E & ~3
    row0 = np.concatenate([[0], np.cumsum([c["DBSize"] for c in cfgs])]).astype(np.uint64)
    out = np.zeros((len(parts), E), dtype=np.uint64)
    for p, c in enumerate(cfgs):
        sel = np.where(parts == p)[0]
        if not len(sel) or not EX:
            continue
        ss = c["SetSize"]
        r = np.arange(ss, dtype=np.uint64)[None, :] * np.uint64(c["ChunkSize"]) + offs[sel, :ss]
        keep = r < c["DBSize"]
        rows = db[np.where(keep, r + row0[p], 0), :EX]
        rows[~keep] = 0
        out[sel, :EX] = np.bitwise_xor.reduce(rows, axis=1)
    return out


def random_sets(cfgs, parts, stride, rng):
    """Offsets below each set's ChunkSize in its first SetSize places, garbage after."""
    offs = rng.integers(2**31, 2**32, size=(len(parts), stride), dtype=np.uint32)
    for p, c in enumerate(cfgs):
        sel = np.where(np.asarray(parts) == p)[0]
        offs[sel, :c["SetSize"]] = rng.integers(0, c["ChunkSize"], size=(len(sel), c["SetSize"]), dtype=np.uint32)
    return offs


def raw_call(pir, parts, offs, out, stride=None, nq=None):
    """The C call itself: (return code, message)."""
    import pacmann_amd as pm
    parts = np.ascontiguousarray(parts, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint32)
    rc = pm.lib().pm_batchpir_server_answer(pir.h, parts.ctypes.data_as(pm.u32p), offs.ctypes.data_as(pm.u32p),
                                            offs.shape[1] if stride is None else stride,
                                            len(parts) if nq is None else nq, out.ctypes.data_as(pm.u64p))
    return rc, pm.lib().pm_last_error()


# ---------------------------------------------------------------------------
# 1. generic batch PIR, partitions of different length
# ---------------------------------------------------------------------------
# E 8: whole 16-B segments; E 6: E & ~3 = 4, words 4 and 5 stay zero; E 80: the graph entry's size (40 segments,
# 6 row slices); E 5 (beyond the three sizes asked for): an odd entry, rows only 8-B aligned, the 8-B instance
@pytest.mark.parametrize("E", [8, 6, 80, 5])
def test_partitions_of_different_length(ctx, E):
    import pacmann_amd as pm
    N, B = 40_003, 16
    raw = rand_db(N, E, seed=E)
    pir = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    cfgs = subconfigs(pir)
    P = len(cfgs)
    assert P == 8 and cfgs[-1]["DBSize"] < cfgs[0]["DBSize"]   # the last partition is shorter
    assert pir.max_set_size == max(c["SetSize"] for c in cfgs)
    stride = pir.max_set_size + 3
    rng = np.random.default_rng(100 + E)
    parts = rng.permutation(np.arange(64) % P).astype(np.uint32)   # 8 sets per partition, shuffled
    offs = random_sets(cfgs, parts, stride, rng)
    last = np.where(parts == P - 1)[0]
    zero_set, top_set = np.where(parts == 2)[0][0], last[0]
    offs[zero_set, :cfgs[2]["SetSize"]] = 0
    offs[top_set, :cfgs[-1]["SetSize"]] = cfgs[-1]["ChunkSize"] - 1
    keep = in_range(cfgs, parts, offs)
    skipped = np.array([cfgs[p]["SetSize"] for p in parts]) - keep.sum(axis=1)
    assert skipped[top_set] > 0 and (skipped[last] > 0).sum() >= 2   # offsets past the last partition's DBSize
    ctx.timing_reset()
    ctx.timing(1)
    try:
        got = pir.ServerAnswer(parts, offs)
        launches, _, alg_bytes = ctx.timing_get("server_answer")
    finally:
        ctx.timing(0)
    want = private_query(raw, E, cfgs, parts, offs)
    assert got.dtype == np.uint64 and got.shape == (64, E)
    assert np.array_equal(got, want)
    assert not got[:, E & ~3:].any()
    assert launches == 1 and alg_bytes == keep.sum() * (E & ~3) * 8   # rows gathered x bytes read per row
    assert ctx.timing_get("host_server_answer_packed")[0] == 0


# ---------------------------------------------------------------------------
# 2. nq edges
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny(ctx):
    import pacmann_amd as pm
    N, E, B = 4096, 4, 4
    raw = rand_db(N, E, seed=77)
    pir = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    return pir, raw, E, subconfigs(pir)


@pytest.mark.parametrize("nq", [1, 2, 65_536 + 1, 0])
def test_nq_edges(tiny, nq):
    pir, raw, E, cfgs = tiny
    rng = np.random.default_rng(nq)
    parts = rng.integers(0, len(cfgs), size=nq, dtype=np.uint32)
    offs = random_sets(cfgs, parts, pir.max_set_size, rng) if nq else np.zeros((0, pir.max_set_size), np.uint32)
    got = pir.ServerAnswer(parts, offs)
    assert got.shape == (nq, E)
    assert np.array_equal(got, private_query(raw, E, cfgs, parts, offs))


def test_nq_zero_touches_nothing(tiny):
    """nq == 0 returns 0 whatever else is passed, NULL pointers included."""
    import pacmann_amd as pm
    pir = tiny[0]
    out = np.full(8, 0xA5A5, dtype=np.uint64)
    assert pm.lib().pm_batchpir_server_answer(pir.h, None, None, 0, 0, out.ctypes.data_as(pm.u64p)) == 0
    assert pm.lib().pm_batchpir_server_answer(pir.h, None, None, 0, 0, None) == 0
    assert (out == 0xA5A5).all()


def test_refusals_leave_out_untouched(tiny):
    pir, raw, E, cfgs = tiny
    rng = np.random.default_rng(5)
    ss = pir.max_set_size
    parts = np.array([0, 1, 0], dtype=np.uint32)
    offs = random_sets(cfgs, parts, ss, rng)
    out = np.full((3, E), 0xA5A5, dtype=np.uint64)
    bad_part = parts.copy()
    bad_part[2] = len(cfgs)
    bad_off = offs.copy()
    bad_off[1, cfgs[1]["SetSize"] - 1] = cfgs[1]["ChunkSize"]
    cases = [
        (lambda: raw_call(pir, parts, offs, out, stride=ss - 1), b"stride must be >= the largest SetSize"),
        (lambda: raw_call(pir, bad_part, offs, out), b"partition out of range"),
        (lambda: raw_call(pir, parts, bad_off, out), b"offset out of range"),
    ]
    for i, (call, text) in enumerate(cases):
        rc, msg = call()
        assert rc == PM_EINVAL and msg.startswith(text), (i, rc, msg)
        assert (out == 0xA5A5).all(), i
    with pytest.raises(RuntimeError, match="offset out of range"):
        pir.ServerAnswer(parts, bad_off)
    rc, _ = raw_call(pir, parts, offs, out)   # and the same arguments, mended, are answered
    assert rc == 0 and np.array_equal(out, private_query(raw, E, cfgs, parts, offs))


# ---------------------------------------------------------------------------
# 3. hint parity: the call against the client side, without the numpy checker
# ---------------------------------------------------------------------------
def test_hint_parity(ctx, oracle):
    """A fresh primary hint j is the XOR of the rows of its set, and its set is
    PRF(key, tag j, chunk i) & (ChunkSize - 1) for every chunk i (pir.go:267-301),
    so the server's answer for that set is the hint's parity."""
    import pacmann_amd as pm
    N, E, B = 30_001, 8, 8
    raw = rand_db(N, E, seed=31)
    srv = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    cli = srv.Client(SEED + 1)
    cli.Preprocessing()
    for p in (1, len(subconfigs(srv)) - 1):   # a full partition and the shorter last one
        c = cli.SubConfig(p)
        st = cli.export_state(p)
        ss, cs = c["SetSize"], c["ChunkSize"]
        hints = np.random.default_rng(p).choice(c["PrimaryHintNum"], size=16, replace=False)
        assert np.array_equal(st["primary_tag"][hints], hints.astype(np.uint64))   # untouched
        offs = np.zeros((16, srv.max_set_size), dtype=np.uint32)
        for k, j in enumerate(hints):
            v = oracle.prf_batch(st["round_keys"], np.full(ss, j, dtype=np.uint64), np.arange(ss, dtype=np.uint64))
            offs[k, :ss] = (v & np.uint64(cs - 1)).astype(np.uint32)
        want = st["primary_parity"].reshape(-1, E)[hints]
        assert want.any()
        for h in (srv, cli):
            assert np.array_equal(h.ServerAnswer(np.full(16, p, dtype=np.uint32), offs), want)


# ---------------------------------------------------------------------------
# 4. graph server: the packed row image
# ---------------------------------------------------------------------------
@pytest.fixture
def options():
    import pacmann_amd as pm
    try:
        yield pm.set_option
    finally:
        pm.set_option("answer_pack", -1)


def graph_raw(v, g):
    """PIRGraphInfo's DB: row r = the vector's f32 words, then the neighbour ids."""
    return np.concatenate([v.view(np.uint32), g], axis=1).copy().view(np.uint64).ravel()


def graph_answers(ctx, v, g, parts_offs=None):
    """A private graph made with skip_prep (no hints are built): (answers, checker's
    answers, launches that read the packed image)."""
    import pacmann_amd as pm
    gi = pm.PIRGraphInfo(v, g, skip_prep=True, pir_seed=SEED, search_seed=3, ctx=ctx)
    gi.Preprocess()
    pir = gi.PIR
    cfgs = subconfigs(pir)
    rng = np.random.default_rng(9)
    parts = rng.permutation(np.arange(48) % len(cfgs)).astype(np.uint32)
    offs = random_sets(cfgs, parts, pir.max_set_size + 1, rng)
    before = ctx.timing_get("host_server_answer_packed")[0]
    got = pir.ServerAnswer(parts, offs)
    packed = ctx.timing_get("host_server_answer_packed")[0] - before
    E = (v.shape[1] + g.shape[1]) // 2
    return got, private_query(graph_raw(v, g), E, cfgs, parts, offs), packed


def test_graph_server(ctx, options):
    n, dim, m = 4099, 128, 32
    rng = np.random.default_rng(44)
    g = rng.integers(0, n, size=(n, m), dtype=np.uint32)
    v_int = rng.integers(0, 256, size=(n, dim)).astype(np.float32)   # f32 of a byte: the low half of every word is zero
    assert not (v_int.view(np.uint32) & 0xffff).any()
    options("answer_pack", 1)
    got1, want, packed1 = graph_answers(ctx, v_int, g)
    options("answer_pack", 0)
    got0, want0, packed0 = graph_answers(ctx, v_int, g)
    assert np.array_equal(want, want0) and want.any()
    assert np.array_equal(got1, want) and np.array_equal(got0, want)
    assert packed1 > 0 and packed0 == 0
    options("answer_pack", 1)
    v_f = rng.random((n, dim), dtype=np.float32)   # low halves in use: the server builds no packed image
    assert (v_f.view(np.uint32) & 0xffff).any()
    got, want, packed = graph_answers(ctx, v_f, g)
    assert np.array_equal(got, want) and packed == 0


# ---------------------------------------------------------------------------
# 5. no client state moves
# ---------------------------------------------------------------------------
STATE_KEYS = ["round_keys", "primary_tag", "primary_parity", "primary_pp", "backup_tag",
              "backup_parity", "repl_idx", "repl_val", "hist"]


def snapshot(pir, P):
    s = pir.stats()
    s.pop("PreprocessingTime")   # wall clock: differs between two handles, compared on one handle below
    return [pir.export_state(p) for p in range(P)], s, [pir.SubConfig(p) for p in range(P)]


def assert_snap_equal(a, b):
    for p, (x, y) in enumerate(zip(a[0], b[0])):
        for k in STATE_KEYS:
            assert np.array_equal(x[k], y[k]), (p, k)
    assert a[1] == b[1] and a[2] == b[2]   # batch stats; every partition's config with its FinishedQueryNum


def test_client_state_does_not_move(ctx):
    import pacmann_amd as pm
    N, E, B = 20_000, 8, 8
    raw = rand_db(N, E, seed=51)
    A = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    Bh = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    A.Preprocessing()
    Bh.Preprocessing()
    cfgs = subconfigs(A)
    P = len(cfgs)
    rng = np.random.default_rng(6)
    parts = rng.integers(0, P, size=40, dtype=np.uint32)
    offs = random_sets(cfgs, parts, A.max_set_size, rng)
    want = private_query(raw, E, cfgs, parts, offs)
    ids = [rng.integers(0, N, size=B).astype(np.uint64) for _ in range(3)]
    ids[2][:3] = ids[0][:3]   # repeats: the local cache answers

    def serve():
        before, t = snapshot(A, P), A.stats()["PreprocessingTime"]
        assert np.array_equal(A.ServerAnswer(parts, offs), want)
        assert_snap_equal(snapshot(A, P), before)
        assert A.stats()["PreprocessingTime"] == t

    assert_snap_equal(snapshot(A, P), snapshot(Bh, P))
    ra, rb = [A.QueryWithMask(ids[0])], [Bh.QueryWithMask(ids[0])]
    serve()
    for q in ids[1:]:   # the second batch, in two calls with the server role between and after them
        ra.append(A.QueryWithMask(q))
        serve()
        rb.append(Bh.QueryWithMask(q))
    for (oa, ka), (ob, kb) in zip(ra, rb):
        assert np.array_equal(oa, ob) and np.array_equal(ka, kb)
    assert ra[0][1].any()
    assert_snap_equal(snapshot(A, P), snapshot(Bh, P))


# ---------------------------------------------------------------------------
# 6. other handles
# ---------------------------------------------------------------------------
def test_other_handles(ctx):
    import pacmann_amd as pm
    N, E, B = 12_345, 6, 8
    raw = rand_db(N, E, seed=61)
    srv = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx)
    srv.Preprocessing()
    cfgs = subconfigs(srv)
    P = len(cfgs)
    rng = np.random.default_rng(8)
    parts = rng.permutation(np.arange(32) % P).astype(np.uint32)
    offs = random_sets(cfgs, parts, srv.max_set_size + 2, rng)
    want = private_query(raw, E, cfgs, parts, offs)
    assert np.array_equal(srv.ServerAnswer(parts, offs), want)
    cli = srv.Client(SEED + 9)   # shares the server's DB; its own state was never built
    assert np.array_equal(cli.ServerAnswer(parts, offs), want)
    fresh = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED + 1, ctx=ctx)   # never preprocessed
    assert np.array_equal(fresh.ServerAnswer(parts, offs), want)
    for shard in (0, 1):   # a shard holds partitions p % 2 == shard, packed: another row0 than the whole DB's
        sh = pm.SimpleBatchPianoPIR(N, E * 8, B, raw, 8, seed=SEED, ctx=ctx, shard=shard, nshards=2)
        assert sh.max_set_size == srv.max_set_size
        own = parts % 2 == shard
        assert np.array_equal(sh.ServerAnswer(parts[own], offs[own]), want[own])
        out = np.full((len(parts), E), 0xA5A5, dtype=np.uint64)
        rc, msg = raw_call(sh, parts, offs, out)
        assert rc == PM_EINVAL and msg.startswith(b"partition not on this shard"), (rc, msg)
        assert (out == 0xA5A5).all()

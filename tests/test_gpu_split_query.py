"""The client role of a two-party round: QueryBegin -> ServerAnswer -> QueryFinish
(pm_batchpir_client_begin / pm_batchpir_server_answer / pm_batchpir_client_finish).

Three handles over one DB: a server that is never preprocessed, client A driven
by the three-call round and client B, created with the same seed, driven by
QueryWithMask.  After every batch A and B agree bit for bit in responses, success
flags, batch counters and every partition's exported state, and both agree with
the oracle's SimpleBatchPianoPIR (responses per batch, state and counters at the
end), as tests/test_gpu_step_forms.py compares.  Shapes and inputs are that
file's: every run holds a failed sub-query, an id repeated in a batch, a local
cache hit and a dummy-padded slot.  Every comparison is exact (XORs, indices).
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_parity import SEED, STATE_KEYS
from tests.test_gpu_step_forms import BY_NAME, Case, FORMS, MATCH, branch_counts, form_counts, inputs, oracle_run

pytestmark = pytest.mark.gpu

PM_EINVAL = -1
STAT_KEYS = ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount", "SupportBatchNum", "PartitionNum",
             "PartitionSize", "DBSize", "DBEntrySize", "BatchSize")
OPEN = "a split query is open"
BUDGET = "partition at its query budget: preprocess first"


def snapshot(c, P):
    return ({k: c.stats()[k] for k in STAT_KEYS}, [c.export_state(p) for p in range(P)])


def assert_same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for p, (x, y) in enumerate(zip(a[1], b[1])):
        for k in STATE_KEYS:
            assert np.array_equal(x[k], y[k]), (what, p, k)


def twins(ctx, N, E, B, F, db, seed=SEED):
    """(server never preprocessed, client A, client B of the same seed), A and B preprocessed."""
    import pacmann_amd as pm
    server = pm.SimpleBatchPianoPIR(N, E * 8, B, db, F, seed=seed + 999, ctx=ctx)
    a, b = server.Client(seed), server.Client(seed)
    a.Preprocessing()
    b.Preprocessing()
    return server, a, b


def check_sets(server, cfgs, osubs, parts, offs, ans):
    """Test 2: the sets are well-formed and the server's answers are the oracle's PrivateQuery of them."""
    assert parts.dtype == np.uint32 and offs.dtype == np.uint32 and offs.shape == (len(parts), server.max_set_size)
    assert (np.diff(parts.astype(np.int64)) >= 0).all()   # partition-major
    for s, p in enumerate(parts.tolist()):
        ss, cs = cfgs[p]["SetSize"], cfgs[p]["ChunkSize"]
        assert (offs[s, :ss] < cs).all(), s
        assert not offs[s, ss:].any(), s
        assert np.array_equal(osubs[p].PrivateQuery(offs[s, :ss]), ans[s]), s


def split_round(server, a, ids, cfgs=None, osubs=None, spoil=None):
    parts, offs = a.QueryBegin(ids)
    ans = server.ServerAnswer(parts, offs)
    if cfgs is not None:
        check_sets(server, cfgs, osubs, parts, offs, ans)
    if spoil is not None:
        ans = spoil(parts, ans)
    out, ok = a.QueryFinish(ans)
    return out, ok, len(parts)


def run_twins(ctx, oracle, N, E, B, F, db, ids, want=None, check=True):
    """ids [batches, n].  Returns (nq per batch, max sets, A, B, server)."""
    server, a, b = twins(ctx, N, E, B, F, db)
    P = a.Config()["PartitionNum"]
    cfgs = [a.SubConfig(p) for p in range(P)]
    o = oracle.SimpleBatchPianoPIR(N, E * 8, B, db, F, seed=1) if check else None   # the DB side only: not preprocessed
    osubs = [o.sub(p) for p in range(P)] if check else None
    nqs = []
    for bi in range(len(ids)):
        out, ok, nq = split_round(server, a, ids[bi], cfgs if check else None, osubs)
        outb, okb = b.QueryWithMask(ids[bi])
        nqs.append(nq)
        assert np.array_equal(out, outb) and np.array_equal(ok, okb), bi
        if want is not None:
            assert np.array_equal(out, want[bi]), bi
        assert_same(snapshot(a, P), snapshot(b, P), bi)
    return nqs, P * (ids.shape[1] // P), a, b, server


GRAPH = dict(N=40_003, E=80, B=16, F=8, n=48, batches=3)
_graph_ref = {}


def graph_inputs(oracle):
    """The graph-entry shape (E 80 words, partitions of different length), its ids planted as inputs() plants
    them, and the oracle's run of them: built once."""
    if not _graph_ref:
        g = GRAPH
        db = np.random.default_rng(8080).integers(0, 2**64, size=g["N"] * g["E"], dtype=np.uint64)
        ids = np.random.default_rng(81).integers(0, g["N"], size=(g["batches"], g["n"]), dtype=np.uint64)
        ids[:, 3] = ids[:, 1]
        ids[1:, 0] = ids[0, 0]
        ids[1:, 2] = ids[0, 2]
        o = oracle.SimpleBatchPianoPIR(g["N"], g["E"] * 8, g["B"], db, g["F"], seed=SEED)
        o.Preprocessing()
        want = np.stack([o.Query(ids[b])[0] for b in range(g["batches"])])
        P = o.stats()["PartitionNum"]
        state = [o.sub(p).export_state() for p in range(P)]
        _graph_ref.update(db=db, ids=ids, want=want, state=state, stats=o.stats())
    return _graph_ref


# ---------------------------------------------------------------------------
# 1 + 2. twin equality, the oracle, well-formed sets
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unfused-W2", "unfused-W1", "gather-W2", "step-nhelp3-W2"])
def test_twin_equals_query_and_oracle(request, oracle, name):
    case = BY_NAME[name]
    ctx = request.getfixturevalue(case.fixture)   # both fusion settings: the split path ignores them
    db, ids, _ = inputs(case)
    want, state, stats, _ = oracle_run(oracle, case)
    assert all(branch_counts(case, ids, want).values())
    nqs, cap, a, b, _ = run_twins(ctx, oracle, case.N, case.E, 2 * case.P, case.F, db, ids[:, 0], want[:, 0])
    assert min(nqs) < cap and max(nqs) <= cap, (nqs, cap)   # a cached / repeated / failed sub-query sent nothing
    for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
        assert a.stats()[key] == stats[0][key], key
    for p in range(case.P):
        got = a.export_state(p)
        for k in STATE_KEYS:
            assert np.array_equal(got[k], state[0][p][k]), (p, k)


def test_twin_graph_entry_shape(ctx, oracle):
    g, ref = GRAPH, graph_inputs(oracle)
    nqs, cap, a, b, _ = run_twins(ctx, oracle, g["N"], g["E"], g["B"], g["F"], ref["db"], ref["ids"], ref["want"])
    assert cap == 48 and min(nqs) < cap, nqs
    for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
        assert a.stats()[key] == ref["stats"][key], key
    for p, st in enumerate(ref["state"]):
        got = a.export_state(p)
        for k in STATE_KEYS:
            assert np.array_equal(got[k], st[k]), (p, k)


# ---------------------------------------------------------------------------
# 3. a dummy set's answer row is not read
# ---------------------------------------------------------------------------
def test_dummy_answers_are_not_read(ctx, oracle):
    case = BY_NAME["unfused-W2"]
    db, ids, _ = inputs(case)
    want, _, _, _ = oracle_run(oracle, case)
    q = ids[0, 0]
    server, a, b = twins(ctx, case.N, case.E, 2 * case.P, case.F, db)
    # the padded slots, from the ids: partition p has qn - (its ids) of them, the last slots of the partition; in a
    # first batch every dummy sends a set, so they are the last sets of the partition
    cnt = np.bincount((q // case.rows).astype(np.int64), minlength=case.P)
    ndummy = np.maximum(case.qn - cnt, 0)
    assert ndummy.sum() > 0
    spoiled = []

    def spoil(parts, ans):
        ans = ans.copy()
        for p in range(case.P):
            sel = np.where(parts == p)[0]
            assert len(sel) >= ndummy[p]
            rows = sel[len(sel) - ndummy[p]:]
            ans[rows] = np.random.default_rng(p).integers(0, 2**64, size=(len(rows), case.E), dtype=np.uint64)
            spoiled.extend(rows.tolist())
        return ans

    out, ok, _ = split_round(server, a, q, spoil=spoil)
    assert len(spoiled) == ndummy.sum()
    outb, okb = b.QueryWithMask(q)
    assert np.array_equal(out, outb) and np.array_equal(ok, okb) and np.array_equal(out, want[0, 0])
    assert_same(snapshot(a, case.P), snapshot(b, case.P), "dummy")


# ---------------------------------------------------------------------------
# 4. counters
# ---------------------------------------------------------------------------
def test_counters(ctx):
    case = BY_NAME["step-nhelp3-W2"]   # a shape QueryWithMask answers with k_step on this context
    db, ids, _ = inputs(case)
    server, a, _ = twins(ctx, case.N, case.E, 2 * case.P, case.F, db)
    ctx.timing_reset()
    ctx.timing(1)
    try:
        for b in range(2):
            split_round(server, a, ids[b, 0])
        got = form_counts(ctx)
        assert ctx.timing_get("client_sets")[0] == 2 and ctx.timing_get("client_finish")[0] == 2
        assert ctx.timing_get("server_answer")[0] == 2
    finally:
        ctx.timing(0)
    assert ctx.timing_get("host_client_begin")[0] == 2 and ctx.timing_get("host_client_finish")[0] == 2
    want = dict.fromkeys(FORMS + tuple(MATCH) + ("nhelp",), 0)
    want["match"] = want["resolve_g"] = 2
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


# ---------------------------------------------------------------------------
# 5. contract
# ---------------------------------------------------------------------------
def raw_begin(pir, ids, cap=None, stride=None):
    import pacmann_amd as pm
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    full = int(pm.lib().pm_batchpir_client_max_sets(pir.h, len(ids)))
    cap = full if cap is None else cap
    stride = pir.max_set_size if stride is None else stride
    parts = np.full(max(cap, 1), 0xABAB, dtype=np.uint32)
    offs = np.full((max(cap, 1), max(stride, 1)), 0xABAB, dtype=np.uint32)
    nq = pm.u64(12345)
    rc = pm.lib().pm_batchpir_client_begin(pir.h, ids.ctypes.data_as(pm.u64p), len(ids), parts.ctypes.data_as(pm.u32p),
                                           offs.ctypes.data_as(pm.u32p), stride, cap, C.byref(nq))
    msg = pm.lib().pm_last_error().decode()
    if rc:
        assert nq.value == 12345 and (parts == 0xABAB).all() and (offs == 0xABAB).all()   # a refusal writes nothing
    return rc, msg, parts[:nq.value], offs[:nq.value]


def raw_finish(pir, ans, nq, n):
    import pacmann_amd as pm
    ans = np.ascontiguousarray(ans, dtype=np.uint64)
    out = np.full((n, pir.E), 0xA5A5, dtype=np.uint64)
    ok = np.full(n, 7, dtype=np.uint8)
    rc = pm.lib().pm_batchpir_client_finish(pir.h, ans.ctypes.data_as(pm.u64p), nq, out.ctypes.data_as(pm.u64p),
                                            ok.ctypes.data_as(C.POINTER(C.c_uint8)))
    msg = pm.lib().pm_last_error().decode()
    if rc:
        assert (out == 0xA5A5).all() and (ok == 7).all()
    return rc, msg, out, ok.astype(bool)


def test_contract(ctx, oracle):
    import pacmann_amd as pm
    case = BY_NAME["unfused-W2"]
    db, ids, _ = inputs(case)
    q0, q1 = ids[0, 0], ids[1, 0]
    P, n = case.P, case.n
    server, a, b = twins(ctx, case.N, case.E, 2 * case.P, case.F, db)
    other = server.Client(SEED + 5)
    other.Preprocessing()
    grp = pm.BatchPIRGroup([a, other])
    full = int(pm.lib().pm_batchpir_client_max_sets(a.h, n))
    assert full == P * (n // P)

    def refused(call, text):
        before = (snapshot(a, P), snapshot(other, P))
        rc, msg = call()
        assert rc == PM_EINVAL and text in msg, (rc, msg)
        assert_same(snapshot(a, P), before[0], text)
        assert_same(snapshot(other, P), before[1], text)

    def wrapped(fn):   # a Python wrapper's RuntimeError as (code, message)
        def call():
            try:
                fn()
            except RuntimeError as e:
                return PM_EINVAL if f"error {PM_EINVAL}:" in str(e) else 0, str(e)
            return 0, ""
        return call

    # closed: (a) finish with no open query; (e) cap one too small; (f) stride one too small; ids, qn
    refused(lambda: raw_finish(a, np.zeros((1, case.E)), 1, n)[:2], "no split query is open")
    refused(lambda: raw_begin(a, q0, cap=full - 1)[:2], "cap must be >=")
    refused(lambda: raw_begin(a, q0, stride=a.max_set_size - 1)[:2], "stride must be >=")
    refused(lambda: raw_begin(a, np.array([case.N] * n))[:2], ">= DBSize")
    refused(lambda: raw_begin(a, q0[:P - 1])[:2], "n / PartitionNum")
    # ... and above the step's sub-queries per partition (the refusal names the limit)
    limit = int(raw_begin(a, q0[:P - 1])[1].split("[1, ")[1].split("]")[0])
    assert limit >= 129   # tests/test_gpu_step_forms.py answers 129 per partition in one step
    too_many = (np.arange((limit + 1) * P, dtype=np.uint64) % P) * case.rows
    refused(lambda: raw_begin(a, too_many)[:2], "n / PartitionNum")
    # open
    rc, msg, parts, offs = raw_begin(a, q0)
    assert rc == 0, msg
    nq = len(parts)
    refused(lambda: raw_begin(a, q0)[:2], OPEN)                                           # (b)
    refused(wrapped(lambda: a.QueryWithMask(q0)), OPEN)                                   # (c)
    refused(wrapped(lambda: a.Query(q0)), OPEN)
    refused(wrapped(lambda: grp.QueryWithMask(np.stack([q0, q0]))), OPEN)
    refused(wrapped(lambda: a.DummyPreprocessing()), OPEN)
    ans = server.ServerAnswer(parts, offs)
    refused(lambda: raw_finish(a, np.zeros((nq + 1, case.E)), nq + 1, n)[:2], "nq is not the number of sets")   # (d)
    refused(lambda: raw_finish(a, ans, nq - 1, n)[:2], "nq is not the number of sets")
    # (g) the server role on the client's own handle while open: allowed, the same answers, nothing of the round moves
    assert np.array_equal(a.ServerAnswer(parts, offs), ans)
    rc, msg, out, ok = raw_finish(a, ans, nq, n)
    assert rc == 0, msg
    outb, okb = b.QueryWithMask(q0)
    assert np.array_equal(out, outb) and np.array_equal(ok, okb)
    assert_same(snapshot(a, P), snapshot(b, P), "after (g)")
    # (h) Preprocessing while open closes the query: the next begin succeeds and the twin agrees again
    a.QueryBegin(q1)
    a.Preprocessing()
    b.Preprocessing()
    refused(lambda: raw_finish(a, np.zeros((1, case.E)), 1, n)[:2], "no split query is open")
    out, ok, _ = split_round(server, a, q1)
    outb, okb = b.QueryWithMask(q1)
    assert np.array_equal(out, outb) and np.array_equal(ok, okb)
    assert_same(snapshot(a, P), snapshot(b, P), "after (h)")


def test_shard_and_envelope_are_refused(ctx):
    """The handle-shape refusals, before any HIP call (the handles are not even preprocessed): a shard handle,
    and entries above the new kernels' 256 words.  (A SetSize above 1,024 needs partitions of millions of rows:
    not built here; it is the same host comparison, of Engine::maxSS.)"""
    import pacmann_amd as pm
    P, rows = 2, 500
    for E, kw, text in ((8, dict(shard=0, nshards=2), "shard handles"), (257, {}, "DBEntrySize <= 256")):
        db = np.random.default_rng(E).integers(0, 2**64, size=P * rows * E, dtype=np.uint64)
        h = pm.SimpleBatchPianoPIR(P * rows, E * 8, 2 * P, db, 4, seed=SEED, ctx=ctx, **kw)
        rc, msg, _, _ = raw_begin(h, np.array([1, rows + 1, 2, rows + 2], dtype=np.uint64))
        assert rc == PM_EINVAL and text in msg, (E, rc, msg)
        rc, msg, _, _ = raw_finish(h, np.zeros((1, E)), 1, 4)
        assert rc == PM_EINVAL and "no split query is open" in msg, (E, rc, msg)


def test_two_wrappers_of_one_handle(ctx):
    """PIRGraphInfo.PIR makes a new wrapper object on every access: begin through one and finish through another
    is the same round (the pending size is the handle's, not the wrapper's), and a finish with no begin on the
    handle is refused without a call that could write past a guessed buffer."""
    import pacmann_amd as pm
    rng = np.random.default_rng(6)
    nv, dim, m = 3000, 8, 8
    vec = rng.integers(0, 255, size=(nv, dim)).astype(np.float32)
    graph = rng.integers(0, nv, size=(nv, m), dtype=np.uint32)
    ga = pm.PIRGraphInfo(vec, graph, pir_seed=4, search_seed=4, ctx=ctx)
    gb = pm.PIRGraphInfo(vec, graph, pir_seed=4, search_seed=4, ctx=ctx)
    ga.Preprocess()
    gb.Preprocess()
    P = ga.PIR.Config()["PartitionNum"]
    assert ga.PIR is not ga.PIR
    with pytest.raises(RuntimeError, match="no split query is open"):
        ga.PIR.QueryFinish(np.zeros((1, ga.PIR.E), dtype=np.uint64))
    for _ in range(2):
        q = rng.integers(0, nv, size=3 * P, dtype=np.uint64)
        parts, offs = ga.PIR.QueryBegin(q)
        out, ok = ga.PIR.QueryFinish(ga.PIR.ServerAnswer(parts, offs))
        assert out.shape == (3 * P, ga.PIR.E) and ok.shape == (3 * P,)
        outb, okb = gb.PIR.QueryWithMask(q)
        assert np.array_equal(out, outb) and np.array_equal(ok, okb) and ok.any()
    assert_same(snapshot(ga.PIR, P), snapshot(gb.PIR, P), "two wrappers")
    # Preprocessing through yet another wrapper closes the query and forgets its size
    ga.PIR.QueryBegin(q)
    ga.PIR.Preprocessing()
    with pytest.raises(RuntimeError, match="no split query is open"):
        ga.PIR.QueryFinish(np.zeros((1, ga.PIR.E), dtype=np.uint64))


def test_graph_pir_handle(ctx):
    """The calls on pm_graph_pir(g): the round equals a twin session's Query, and the graph calls are refused
    while the split query is open."""
    import pacmann_amd as pm
    rng = np.random.default_rng(5)
    nv, dim, m = 3000, 8, 8
    vec = rng.integers(0, 255, size=(nv, dim)).astype(np.float32)
    graph = rng.integers(0, nv, size=(nv, m), dtype=np.uint32)
    ga = pm.PIRGraphInfo(vec, graph, pir_seed=3, search_seed=3, ctx=ctx)
    gb = pm.PIRGraphInfo(vec, graph, pir_seed=3, search_seed=3, ctx=ctx)
    ga.Preprocess()
    gb.Preprocess()
    pa, pb = ga.PIR, gb.PIR
    P = pa.Config()["PartitionNum"]
    q = rng.integers(0, nv, size=2 * P, dtype=np.uint64)
    parts, offs = pa.QueryBegin(q)
    with pytest.raises(RuntimeError, match=OPEN):
        ga.GetVertexInfo(q[:P])
    out, ok = pa.QueryFinish(pa.ServerAnswer(parts, offs))
    outb, okb = pb.QueryWithMask(q)
    assert np.array_equal(out, outb) and np.array_equal(ok, okb) and ok.any()
    assert_same(snapshot(pa, P), snapshot(pb, P), "graph")


# ---------------------------------------------------------------------------
# 6 + 7. across a re-preprocessing; the budget refusal
# ---------------------------------------------------------------------------
SMALL = Case("split-small", (), P=4, rows=2500, E=8, F=4, qn=1, geom=None)


def small_db():
    return np.random.default_rng(2500).integers(0, 2**64, size=SMALL.N * SMALL.E, dtype=np.uint64)


def test_across_a_repreprocessing(ctx):
    """n = PartitionNum: one sub-query per partition, so fqn <= QueriesMadeInPartition < MaxQueryNum - 2 before
    every batch and begin is never refused; the trigger (bq_tail) fires inside finish."""
    c = SMALL
    db = small_db()
    server, a, b = twins(ctx, c.N, c.E, 2 * c.P, c.F, db)
    rng = np.random.default_rng(66)
    maxq = a.SubConfig(0)["MaxQueryNum"]
    after, batches = None, 0
    while after is None or after > 0:
        assert batches <= maxq + 8   # the trigger fires by MaxQueryNum - 2 batches
        q = (np.arange(c.P) * c.rows + rng.integers(0, c.rows, size=c.P)).astype(np.uint64)   # one id per partition
        out, ok, _ = split_round(server, a, q)   # (a refused begin raises)
        outb, okb = b.QueryWithMask(q)
        batches += 1
        assert np.array_equal(out, outb) and np.array_equal(ok, okb), batches
        assert_same(snapshot(a, c.P), snapshot(b, c.P), batches)
        if after is None and a.stats()["PrepCount"] == 2:
            assert b.stats()["PrepCount"] == 2
            after = 4
        elif after is not None:
            after -= 1
    assert a.stats()["PrepCount"] == 2 and batches > 5


def test_budget_refusal(ctx):
    """A partition whose FinishedQueryNum + real sub-queries reaches MaxQueryNum before the batch counter's
    trigger fires makes begin refuse, with nothing changed; after Preprocessing the same ids succeed.
    n = 24 PartitionNum: on this shape (MaxQueryNum 391, about one sub-query in 16 failing) the oracle's run of
    these ids shows the trigger firing first with 6 and with 12 ids per partition (after 65 and 33 batches,
    FinishedQueryNum 352-369), so n was raised as far as the refusal needs: with 24 it comes at the 18th batch."""
    c = SMALL
    db = small_db()
    server, a, b = twins(ctx, c.N, c.E, 2 * c.P, c.F, db)
    rng = np.random.default_rng(67)
    per = 24   # (one step: tests/test_gpu_step_forms.py runs 129 per partition)
    n = per * c.P
    refused_ids = None
    for _ in range(a.stats()["SupportBatchNum"] + 2):
        # distinct ids in every partition: every one a real sub-query that counts
        q = np.concatenate([p * c.rows + rng.choice(c.rows, size=per, replace=False) for p in range(c.P)]).astype(np.uint64)
        before = snapshot(a, c.P)
        rc, msg, parts, offs = raw_begin(a, q)
        if rc:
            assert rc == PM_EINVAL and BUDGET in msg, msg
            assert_same(snapshot(a, c.P), before, "refused begin")
            refused_ids = q
            break
        rcf, msgf, out, ok = raw_finish(a, server.ServerAnswer(parts, offs), len(parts), n)
        assert rcf == 0, msgf
        outb, okb = b.QueryWithMask(q)   # the twin re-preprocesses mid-batch where begin would refuse the next time
        assert np.array_equal(out, outb) and np.array_equal(ok, okb)
    assert refused_ids is not None, "no begin was refused on this shape"
    a.Preprocessing()
    out, ok, _ = split_round(server, a, refused_ids)
    rows = db.reshape(c.N, c.E)[refused_ids.astype(np.int64)]
    assert ok.any() and np.array_equal(out[ok], rows[ok]) and not out[~ok].any()

"""pm_graph_group_*: many private sessions' GetVertexInfo calls
(private-search.go:441-506) answered in one shared step, and their Preprocess
as one launch set.  The contract is exact equivalence: after every group call
each session's outputs, counters, batch-PIR statistics and exported hint state
equal those of an identical session driven alone through
pm_graph_get_vertex_info / pm_graph_preprocess, and the rows equal the
oracle's.

Set A is driven through the group, set B (same seeds) through the
single-session calls.  As in pm_graph_get_vertex_info, a session's ids of one
call are ONE SimpleBatchPianoPIR.Query, so a call has one shared step however
many ids a session brings; "a batch" below is BatchSize (= m) ids."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2_000
SHAPES = [(16, 8), (128, 32)]
STAT_KEYS = ("FinishedBatchNum", "QueriesMadeInPartition", "SupportBatchNum", "PrepCount", "LocalStorage",
             "CommOnline", "CommOffline")
_cache = {}


def _data(dim, m):
    if (dim, m) not in _cache:
        from pacmann_amd.synth import random_graph, sift_like_vectors
        _cache[dim, m] = (sift_like_vectors(N, dim, seed=500 + dim), random_graph(N, m, seed=501 + dim))
    return _cache[dim, m]


def _sessions(pm, v, g, S, seed0):
    """A preprocessed base and S - 1 preprocessed sessions of it, each on a context of its own."""
    base = pm.PIRGraphInfo(v, g, pir_seed=seed0, search_seed=seed0 + 1000, ctx=pm.Context(0))
    base.Preprocess()
    out = [base]
    for i in range(1, S):
        s = base.Session(seed0 + i, seed0 + 1000 + i)
        s.Preprocess()
        out.append(s)
    return out


def _state(s):
    """Everything the contract names besides the outputs: counts, statistics (without wall times), hint state."""
    pir = s.PIR
    st = pir.stats()
    parts = [pir.export_state(p) for p in range(st["PartitionNum"])]
    fqn = [pir.SubConfig(p)["FinishedQueryNum"] for p in range(st["PartitionNum"])]
    return s.counts(), {k: st[k] for k in STAT_KEYS}, fqn, parts


def _same_state(a, b, what):
    ca, sa, fa, pa = _state(a)
    cb, sb, fb, pb = _state(b)
    assert ca == cb, (what, "counts")
    assert sa == sb, (what, "stats")
    assert fa == fb, (what, "FinishedQueryNum")
    for p, (x, y) in enumerate(zip(pa, pb)):
        for k in x:
            assert np.array_equal(x[k], y[k]), (what, "partition", p, k)


def _single(sess, ids, q):
    """The single-session call; (vecs, nbrs, ok, dist or None)."""
    if len(ids) == 0:
        return None
    r = sess.GetVertexInfo(ids, q)
    return r if q is not None else (*r, None)


def _same_out(ga, sb, what):
    if sb is None:
        assert all(x is None or len(x) == 0 for x in ga), what
        return
    for k, (x, y) in enumerate(zip(ga, sb)):
        if x is None or y is None:
            continue
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), (what, k)
    ok = sb[2]
    assert not sb[0][~ok].any() and not sb[1][~ok].any(), what   # ok = 0 rows are zero
    if ga[0] is not None and ga[2] is not None:
        assert not ga[0][~ga[2]].any() and not ga[1][~ga[2]].any(), what


def _round(grp, B, ids, qs, what):
    out = grp.get_vertex_info(ids, qs)
    for s, sess in enumerate(B):
        _same_out(out[s], _single(sess, ids[s], None if qs is None else qs[s]), (what, s))
    for s, (a, b) in enumerate(zip(grp.sessions, B)):
        _same_state(a, b, (what, s))
    return out


def _round_ids(rng, S, n, prev):
    ids = [rng.integers(0, N, size=n) for _ in range(S)]
    for s in range(S):
        if n > 6:
            ids[s][5] = ids[s][1]   # a duplicate inside the call
        if prev is not None and n >= 14 and len(prev[s]) >= 14:
            ids[s][8:12] = prev[s][2:6]   # repeats across rounds: the local cache
    return ids


@pytest.mark.parametrize("dim,m", SHAPES)
@pytest.mark.parametrize("S", [1, 2, 5])
def test_parity_with_oracle_and_single_calls(oracle, dim, m, S):
    import pacmann_amd as pm
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, S, 40), _sessions(pm, v, g, S, 40)
    O = []
    for i in range(S):
        og = oracle.Graph(v, g, pir_seed=40 + i, search_seed=1040 + i)
        og.Preprocess()
        O.append(og)
    grp = pm.PIRGraphGroup(A)
    rng = np.random.default_rng(7 + S)
    prev = None
    for r in range(8):
        ids = _round_ids(rng, S, 3 * m, prev)
        qs = (v[rng.integers(0, N, size=S)] + rng.normal(0, 8, (S, dim))).astype(np.float32)
        out = _round(grp, B, ids, qs, ("round", r))
        for s in range(S):
            vo, no = O[s].GetVertexInfo(ids[s])
            va, na, ok, d = out[s]
            assert np.array_equal(va.view(np.uint32), vo.view(np.uint32)), (r, s)
            assert np.array_equal(na, no), (r, s)
            assert np.array_equal(ok, (no == g[ids[s]]).all(axis=1)), (r, s)
            want = np.where(ok, oracle.l2_batch(qs[s], vo), np.float32(0)).astype(np.float32)
            assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), (r, s)
            assert A[s].counts() == O[s].counts(), (r, s)
        prev = ids
    assert sum(int(o[2].sum()) for o in out) > 0


@pytest.mark.parametrize("dim,m", SHAPES)
def test_ragged_counts(dim, m):
    """0, 1, one batch, one batch + 1 and three batches of ids in one call.
    Each session's ids are one Query (as in the single-session call), so the
    call launches exactly one shared step; the session with 1 id (fewer ids
    than partitions: every id dropped) is served alone, as the single call
    serves it; the session with 0 ids is untouched."""
    import pacmann_amd as pm
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 5, 60), _sessions(pm, v, g, 5, 60)
    grp = pm.PIRGraphGroup(A)
    rng = np.random.default_rng(11)
    before0 = _state(A[0])
    c0 = A[0].ctx
    for r in range(3):
        steps = c0.timing_get("host_gvi_group_steps")[0]
        calls = c0.timing_get("host_gvi_group")[0]
        ids = [rng.integers(0, N, size=k) for k in (0, 1, m, m + 1, 3 * m)]
        qs = rng.normal(100, 30, (5, dim)).astype(np.float32)
        _round(grp, B, ids, qs, ("ragged", r))
        assert c0.timing_get("host_gvi_group_steps")[0] == steps + 1
        assert c0.timing_get("host_gvi_group")[0] == calls + 1
    after0 = _state(A[0])
    assert before0[:3] == after0[:3]
    for x, y in zip(before0[3], after0[3]):
        for k in x:
            assert np.array_equal(x[k], y[k]), k
    # nobody brings ids: nothing runs, nothing moves
    steps = c0.timing_get("host_gvi_group_steps")[0]
    out = grp.get_vertex_info([[]] * 5, None)
    assert all(len(o[0]) == 0 for o in out) and c0.timing_get("host_gvi_group_steps")[0] == steps


@pytest.mark.parametrize("dim,m", SHAPES)
def test_duplicates_and_drops(dim, m):
    import pacmann_amd as pm
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 2, 80), _sessions(pm, v, g, 2, 80)
    grp = pm.PIRGraphGroup(A)
    P = A[0].PIR.stats()["PartitionNum"]
    PS = A[0].PIR.stats()["PartitionSize"]
    rng = np.random.default_rng(13)
    dup = rng.integers(0, N, size=3 * m)
    dup[7] = dup[2]
    # 2 P ids of partition 0: two sub-queries per partition, the other 2 P - 2 ids dropped (batch-pir.go:195-200)
    crowd = rng.permutation(min(PS, N))[:2 * P]
    qs = rng.normal(100, 30, (2, dim)).astype(np.float32)
    out = _round(grp, B, [dup, crowd], qs, "dups and drops")
    assert np.array_equal(out[0][0][7], out[0][0][2]) and out[0][2][7] == out[0][2][2]
    assert int((~out[1][2]).sum()) >= 2 * P - 2
    _round(grp, B, [crowd, dup], qs, "again, swapped")


def test_general_path():
    """One session of three at a partition's query budget: its bucketing
    leaves the one-step path, it is served alone (steps on its own context),
    the other two still share one step, and all three match set B."""
    import pacmann_amd as pm
    dim, m = SHAPES[0]
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 3, 90), _sessions(pm, v, g, 3, 90)
    grp = pm.PIRGraphGroup(A)
    st = B[1].PIR.stats()
    P, PS = st["PartitionNum"], st["PartitionSize"]
    maxq = min(B[1].PIR.SubConfig(p)["MaxQueryNum"] for p in range(P))
    assert maxq < 400, maxq   # a few hundred ids reach it on this graph
    rng = np.random.default_rng(17)
    order = [p * PS + rng.permutation(min(PS, N - p * PS)) for p in range(P)]
    q1 = rng.normal(100, 30, (3, dim)).astype(np.float32)
    # one fresh id per partition per call: FinishedQueryNum and QueriesMadeInPartition rise by one each,
    # up to three short of the budget (the batch layer re-preprocesses at MaxQueryNum - 2)
    for k in range(maxq - 3):
        ids1 = np.array([order[p][k] for p in range(P)])
        out = grp.get_vertex_info([[], ids1, []], q1)
        _same_out(out[1], _single(B[1], ids1, q1[1]), ("drive", k))
    for s in range(3):
        _same_state(A[s], B[s], ("driven", s))
    fqn = [B[1].PIR.SubConfig(p)["FinishedQueryNum"] for p in range(P)]
    ids1 = np.concatenate([order[p][maxq:maxq + 6] for p in range(P)])
    assert any(f + 6 >= maxq for f in fqn), (fqn, maxq)   # bq_prepare: a partition at its budget
    launches = [s.ctx.timing_get("host_step_launch")[0] for s in A]
    steps = A[0].ctx.timing_get("host_gvi_group_steps")[0]
    ids = [rng.integers(0, N, size=6 * P), ids1, rng.integers(0, N, size=6 * P)]
    _round(grp, B, ids, q1, "budget round")
    after = [s.ctx.timing_get("host_step_launch")[0] for s in A]
    assert after[0] == launches[0] + 1 and after[2] == launches[2]   # sessions 0 and 2: one shared step
    assert after[1] > launches[1]                                     # session 1: its own steps
    assert A[0].ctx.timing_get("host_gvi_group_steps")[0] == steps + 1
    _round(grp, B, [rng.integers(0, N, size=6 * P) for _ in range(3)], q1, "the round after")


def test_mixed_use_and_maintenance():
    """Group call, single call on one member, group call, repeated until the
    batch layer has re-preprocessed (bq_tail's trigger inside a group call)
    and once after a member's own pm_graph_preprocess: all equal set B driven
    by the same sequence of single calls."""
    import pacmann_amd as pm
    dim, m = SHAPES[0]
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 3, 120), _sessions(pm, v, g, 3, 120)
    grp = pm.PIRGraphGroup(A)
    rng = np.random.default_rng(19)
    maxq = B[0].PIR.SubConfig(0)["MaxQueryNum"]
    qn = 6
    rounds = 0
    while B[0].PIR.stats()["PrepCount"] < 2:
        assert rounds <= maxq // qn + 2
        ids = [rng.integers(0, N, size=qn * m // 2) for _ in range(3)]
        qs = rng.normal(100, 30, (3, dim)).astype(np.float32)
        _round(grp, B, ids, qs, ("group", rounds))
        solo = rng.integers(0, N, size=qn * m // 2)
        _same_out(_single(A[1], solo, qs[1]), _single(B[1], solo, qs[1]), ("solo", rounds))
        _same_state(A[1], B[1], ("solo", rounds))
        rounds += 1
    A[2].Preprocess()
    B[2].Preprocess()
    for r in range(2):
        ids = [rng.integers(0, N, size=qn * m // 2) for _ in range(3)]
        _round(grp, B, ids, None, ("after a member's Preprocess", r))


@pytest.mark.parametrize("want", [("dist",), ("nbrs",), ()])
def test_null_outputs(want):
    import pacmann_amd as pm
    dim, m = SHAPES[0]
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 2, 150), _sessions(pm, v, g, 2, 150)
    grp = pm.PIRGraphGroup(A)
    rng = np.random.default_rng(23)
    for r in range(3):
        ids = [rng.integers(0, N, size=3 * m) for _ in range(2)]
        qs = rng.normal(100, 30, (2, dim)).astype(np.float32)
        out = grp.get_vertex_info(ids, qs if "dist" in want else None, want=want)
        for s in range(2):
            ref = B[s].GetVertexInfo(ids[s], qs[s])
            for k, name in enumerate(("vecs", "nbrs", "ok", "dist")):
                if name in want:
                    assert np.array_equal(out[s][k], ref[k]), (r, s, name)
                else:
                    assert out[s][k] is None
            _same_state(A[s], B[s], (r, s))


def test_group_preprocess():
    import pacmann_amd as pm
    dim, m = SHAPES[1]
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 3, 170), _sessions(pm, v, g, 3, 170)
    grp = pm.PIRGraphGroup(A)
    rng = np.random.default_rng(29)
    ids = [rng.integers(0, N, size=3 * m) for _ in range(3)]
    _round(grp, B, ids, None, "before")
    sets = A[0].ctx.timing_get("host_prep_sets")
    grp.preprocess()
    got = A[0].ctx.timing_get("host_prep_sets")
    assert got[0] == sets[0] + 1 and got[1] == sets[1] + 2   # the two sessions of the base: one launch set
    for b in B[1:] + B[:1]:   # the base last: its sessions take their new clients from its current server
        b.Preprocess()
    for s in range(3):
        _same_state(A[s], B[s], ("preprocessed", s))
        for x, y in zip(A[s].GetStartVertex(), B[s].GetStartVertex()):
            assert np.array_equal(x, y)
    _round(grp, B, ids, None, "after")


def test_kernel_forms():
    """A group call on S = 5 counts in the same host_path_* counters as a
    pm_batchpir_group_query of the same shape, on the first session's context
    alone: one launch chain per call, not one per session."""
    import pacmann_amd as pm
    dim, m = SHAPES[1]
    v, g = _data(dim, m)
    A, B = _sessions(pm, v, g, 5, 200), _sessions(pm, v, g, 5, 200)
    names = ["host_path_match", "host_path_match_part", "host_path_match_part8", "host_path_step",
             "host_path_resolve_lds", "host_path_resolve_g", "host_path_mr_s2", "host_path_mr_s4",
             "host_path_mr_general", "host_path_gather", "host_path_answer_p5", "host_path_answer_p",
             "host_path_answer_s", "host_path_answer_g", "host_step_launch"]

    def counts(c):
        return np.array([c.timing_get(k)[0] for k in names])
    for s in A + B:
        s.ctx.timing(2)
    rng = np.random.default_rng(31)
    ids = np.stack([rng.integers(0, N, size=3 * m) for _ in range(5)])
    grp = pm.PIRGraphGroup(A)
    a0 = [counts(s.ctx) for s in A]
    grp.get_vertex_info(list(ids), rng.normal(100, 30, (5, dim)).astype(np.float32))
    da = [counts(s.ctx) - x for s, x in zip(A, a0)]
    pirs = [s.PIR for s in B]
    bg = pm.BatchPIRGroup(pirs)
    b0 = [counts(s.ctx) for s in B]
    bg.QueryWithMask(ids)
    db = [counts(s.ctx) - x for s, x in zip(B, b0)]
    assert da[0].sum() > 1 and da[0][-1] == 1
    assert np.array_equal(da[0], db[0]), dict(zip(names, zip(da[0], db[0])))
    for s in range(1, 5):
        assert not da[s].any() and not db[s].any(), s
    for s in A + B:
        s.ctx.timing(0)

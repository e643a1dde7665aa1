"""The query chain's answer kernel in both forms, in shared batch-PIR steps and
in the device loop.

k_answer_p (two sub-queries per workgroup, pm_query.hip) exists in two forms,
chosen by pm_set_option("answer_waves", 6 / 5): 6 waves per SIMD with six rows
per gather batch, and k_answer_p5 with 5 waves per SIMD and seven rows per
batch.  Both must answer exactly like the CPU oracle.  The kernel is reached
only by shared steps with pre-expanded query sets: at least 128 partitions
(clients x partitions), at least four sub-queries per partition, and every
(client, partition) pair holds the same number, so a step has np * qn
sub-queries with np >= 128, qn >= 4.  The cases are batch-PIR groups
(pm_batchpir_group_query) of exactly 512 = 128 * 4 sub-queries, the least
that takes the kernel, and 645 = 129 * 5, the least odd count (513 = 27 * 19
has no such factorisation): the last workgroup then holds sub-query A alone.

SetSize is ceil(N / ChunkSize) rounded up to a multiple of 4 (pir.go:479-514),
so a SetSize of exactly 7 cannot be configured.  What the batch size can get
wrong is a thread's own row count: a thread of slice sl of nsl gathers rows
sl, sl + nsl, ...; at E = 80 (and 82) words nsl is 3, and the cases below give
per-thread counts of

    SetSize   4: 2 / 1 / 1      below one batch
    SetSize   8: 3 / 3 / 2      (8 = 7 + 1)
    SetSize  20: 7 / 7 / 6      one batch of 6 exactly, 6 + 1, one batch of 7; 20 = 2 * 7 + 6
    SetSize  24: 8 / 8 / 8      7 + 1
    SetSize  40: 14 / 13 / 13   2 * 6 + 1, 2 * 7, 7 + 6
    SetSize 124: 42 / 41 / 41   the SIFT1M shape (124 = 17 * 7 + 5); 7 * 6, 5 * 7 + 6
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20240501
STATE_KEYS = ["round_keys", "primary_tag", "primary_parity", "primary_pp", "backup_tag",
              "backup_parity", "repl_idx", "repl_val", "hist"]
BATCHES = 2

# partition rows -> SetSize (ChunkSize = the power of two >= 2 sqrt(rows))
PART_ROWS = {4: 128, 8: 500, 20: 2500, 24: 3000, 40: 10000, 124: 63000}
# sub-queries per step -> (partitions, clients, sub-queries per partition and client)
STEP = {512: (2, 64, 4), 645: (3, 43, 5)}
F = 4   # FailureProbLog2: PrimaryHintNum = 4 * ChunkSize; about one sub-query in 16 fails

SHAPES = [(ss, 512, 80) for ss in PART_ROWS] + [(20, 645, 80), (124, 645, 80), (24, 512, 82), (20, 645, 82)]

_reference = {}


def _inputs(ss, nsub, E):
    P, S, qn = STEP[nsub]
    N = P * PART_ROWS[ss]
    db = np.random.default_rng(1000 * ss + nsub + E).integers(0, 2**64, size=N * E, dtype=np.uint64)
    rng = np.random.default_rng(7 * ss + nsub)
    ids = rng.integers(0, N, size=(BATCHES, S, P * qn), dtype=np.uint64)
    ids[:, :, 3] = ids[:, :, 1]          # a repeat inside a batch
    ids[1, :, 0] = ids[0, :, 0]          # an id answered in the batch before: the local cache
    seeds = [SEED + 31 * i for i in range(S)]
    return N, db, ids, seeds


def _oracle_run(oracle, ss, nsub, E):
    """Every client's responses per batch and its state after the last one,
    computed once per shape and shared by both forms' cases."""
    key = (ss, nsub, E)
    if key not in _reference:
        P, S, qn = STEP[nsub]
        N, db, ids, seeds = _inputs(ss, nsub, E)
        ors = [oracle.SimpleBatchPianoPIR(N, E * 8, 2 * P, db, F, seed=sd) for sd in seeds]
        for o in ors:
            o.Preprocessing()
        want = np.stack([np.stack([o.Query(ids[b, i])[0] for i, o in enumerate(ors)]) for b in range(BATCHES)])
        state = [[o.sub(p).export_state() for p in range(P)] for o in ors]
        stats = [o.stats() for o in ors]
        for a in (want, *[x[k] for st in state for x in st for k in STATE_KEYS]):
            a.setflags(write=False)
        _reference[key] = (want, state, stats)
    return _reference[key]


@pytest.mark.parametrize("waves", [6, 5])
@pytest.mark.parametrize("ss,nsub,E", SHAPES)
def test_answer_forms_match_oracle(oracle, ss, nsub, E, waves):
    """Both forms of k_answer_p at the SetSizes of the module docstring, at
    exactly 512 sub-queries per step (the least that take the kernel) and 645
    (odd: the last workgroup holds sub-query A alone), E = 80 words and 82 (not
    a multiple of 4: two tail words outside the XOR).  Two batches per client,
    the second after the first one's refresh, with a repeat and a cached id:
    the responses, the success flags (ok: the DB row; not ok: zero) and every
    partition's refreshed client state equal the oracle's bit for bit.  The
    step counters show that every batch was one shared step of the
    k_match_resolve_s -> answer chain, with no client served on its own, and
    the form counters that it was k_match_resolve_s<2,256> and the asked-for
    form of the pair kernel."""
    import pacmann_amd as pm
    from tests.test_gpu_step_forms import assert_forms
    P, S, qn = STEP[nsub]
    assert S * P * qn == nsub
    N, db, ids, seeds = _inputs(ss, nsub, E)
    want, state, stats = _oracle_run(oracle, ss, nsub, E)
    ctx = pm.Context(0)
    pm.set_option("answer_waves", waves)
    try:
        server = pm.SimpleBatchPianoPIR(N, E * 8, 2 * P, db, F, seed=seeds[0], ctx=ctx)
        assert server.Config()["PartitionNum"] == P
        assert server.SubConfig(0)["SetSize"] == ss
        clients = [server] + [server.Client(sd) for sd in seeds[1:]]
        for c in clients:
            c.Preprocessing()
        grp = pm.BatchPIRGroup(clients)
        ctx.timing_reset()
        ctx.timing(2)
        rows = db.reshape(N, E)
        for b in range(BATCHES):
            got, ok = grp.QueryWithMask(ids[b])
            assert np.array_equal(got, want[b]), b
            for i in range(S):
                r = rows[ids[b, i].astype(np.int64)]
                assert np.array_equal(got[i][ok[i]][:, :E & ~3], r[ok[i]][:, :E & ~3]), (b, i)
                assert not got[i][:, E & ~3:].any(), (b, i)   # the words past len & ~3 stay out of the XOR
                assert not got[i][~ok[i]].any(), (b, i)
        ctx.sync()
        ctx.timing(False)
        launches = {k: ctx.timing_get(k)[0] for k in ("match_resolve", "answer", "step", "hint_match", "gather")}
        assert launches == {"match_resolve": BATCHES, "answer": BATCHES, "step": 0, "hint_match": 0, "gather": 0}
        assert_forms(ctx, BATCHES, ("mr_s2", "answer_p5" if waves == 5 else "answer_p"))
        for i, c in enumerate(clients):
            for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
                assert c.stats()[key] == stats[i][key], (i, key)
            for p in range(P):
                a = c.export_state(p)
                for k in STATE_KEYS:
                    assert np.array_equal(a[k], state[i][p][k]), (i, p, k)
    finally:
        ctx.timing(False)
        pm.set_option("answer_waves", -2)


@pytest.mark.parametrize("per_team", [6, 8])
def test_device_loop_answer_form_and_hand_over(oracle, per_team):
    """2 teams x 6 sessions on the 16,384-vertex graph of
    test_search_device_loop_vs_host_loop (96 sub-queries per session and round:
    576 per team step over 6 x 16 = 96 partitions, which k_answer_s answers),
    and 2 teams x 8 sessions (768 over 128 partitions: the least that takes
    k_match_resolve_s -> k_answer_p); three queries, the harness's merged
    maintenance after each.  The entries are 80 words, so the default takes the
    5-wave form.  The device loop and the host loop on fresh sessions with the
    same seeds give the same answers, graph counts, batch-PIR counters and
    probe responses (dummy counters, FinishedQueryNum, the localCache index) as
    each other and as the oracle, and the device run's form counters show
    k_match_part8 -> k_resolve -> k_answer_s for 6 sessions per team and
    k_match_resolve_s<2,256> -> k_answer_p5 for 8.  Then one host-loop call on the device-loop
    sessions: its steps wait for their own completion records, and its answers
    (which continue the sessions' search streams and PIR state) equal the
    oracle's next query."""
    import pacmann_amd as pm
    from pacmann_amd.synth import random_graph, sift_like_vectors
    from tests.test_gpu_step_forms import form_counts
    n, S, NQ = 16384, 2 * per_team, 3
    v = sift_like_vectors(n, 128, seed=71)
    graph = random_graph(n, 32, seed=72)
    seeds = [(80 + i, 90 + i) for i in range(S)]
    rng = np.random.default_rng(75)
    qs = np.stack([np.clip(np.rint(v[rng.integers(0, n, NQ + 1)] + rng.normal(0, 8, (NQ + 1, 128))), 0, 255)
                   .astype(np.float32) for _ in seeds])
    q_loop, q_next = np.ascontiguousarray(qs[:, :NQ]), np.ascontiguousarray(qs[:, NQ:])
    probe = np.random.default_rng(76).integers(0, n, size=96).astype(np.uint64)
    out = {}
    try:
        for mode in (1, 0):
            pm.set_option("device_loop", mode)
            base = pm.PIRGraphInfo(v, graph, pir_seed=1, search_seed=2, ctx=pm.Context(0))
            base.Preprocess()
            sess = [base.Session(p, s) for p, s in seeds]
            for x in sess:
                x.Preprocess()
            for x in sess:
                x.ctx.timing_reset()
            ans, _, _, mt = pm.search_loop_batched(sess, q_loop, 10, 20, 3, 2, 4)
            dev_steps = sum(x.ctx.timing_get("host_dev_steps")[0] for x in sess)
            forms = form_counts([x.ctx for x in sess])
            counts = [x.counts() for x in sess]
            stats = [x.PIR.stats() for x in sess]
            extra = [x.PIR.QueryWithMask(probe) for x in sess]
            pm.set_option("device_loop", 0)   # the hand-over: a host-loop call on these sessions
            nxt, _, _, _ = pm.search_loop_batched(sess, q_next, 10, 20, 3, 2, 4)
            out[mode] = (ans, counts, stats, extra, dev_steps, (mt > 0).all(), nxt, forms)
    finally:
        pm.set_option("device_loop", -1)
    (a1, c1, s1, x1, st1, m1, n1, f1), (a0, c0, s0, x0, st0, m0, n0, _) = out[1], out[0]
    assert st1 == NQ * 20 * 2 and st0 == 0   # every step of the device run on the GPU loop, none of the host run
    # every device step is one hint-search and one answer launch of the team's form (a session's own steps, if
    # any, are engine steps: k_step or k_match -> k_resolve -> k_answer_s)
    if per_team == 8:
        assert f1["mr_s2"] == f1["answer_p5"] == st1, f1
        assert f1["match_part8"] == f1["match_part"] == 0, f1
    else:
        assert f1["match_part8"] == st1 and f1["resolve_g"] >= st1 and f1["answer_s"] >= st1, f1
        assert f1["mr_s2"] == f1["answer_p5"] == 0, f1
    assert f1["mr_s4"] == f1["mr_general"] == f1["answer_p"] == f1["answer_g"] == f1["gather"] == f1["resolve_lds"] == 0, f1
    assert m1 and m0                         # maintenance ran inside both calls
    assert np.array_equal(a1, a0) and np.array_equal(n1, n0)
    assert c1 == c0
    for a, b in zip(s1, s0):
        for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
            assert a[key] == b[key], key
        assert a["PrepCount"] > 2
    for (ra, oa), (rb, ob) in zip(x1, x0):
        assert np.array_equal(ra, rb) and np.array_equal(oa, ob)
    for i, (p, s) in enumerate(seeds):
        o = oracle.Graph(v, graph, pir_seed=p, search_seed=s)
        o.Preprocess()
        oa, _, _ = o.SearchLoop(q_loop[i], 10, 20, 3)
        assert np.array_equal(a1[i], oa), i
        assert c1[i] == o.counts(), i
        po, _ = o.pir().Query(probe)
        assert np.array_equal(x1[i][0], po), i
        on, _, _ = o.SearchLoop(q_next[i], 10, 20, 3)
        assert np.array_equal(n1[i], on), i

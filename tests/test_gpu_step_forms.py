"""Every kernel form of the online query step against the oracle.

Which kernels answer a step is decided by step_plan of pm_query.hip alone
(pm.step_plan shows its answer without a GPU: tests/test_step_plan.py); the one
launch chain of engine_step and group_step_launch (the device loop through it)
counts every launch by its form in the "host_path_*" counters:

  counter        kernel                       selected by
  step           k_step<W> (one launch)       engine_step only: descriptor in the kernel arguments (nsub <= 112,
                                              P <= 32), qn <= 64, PH <= 8,192, 2 nsub + P <= 256, no PM_NO_FUSE;
                                              total_ms = sum of nhelp = min(3, (240 - 2 nsub - P) / nsub), 0 where
                                              E & ~3 > 256; W = 2 for even E, 1 for odd
  match*         k_match / _part / _part8     every step that is neither k_step nor k_match_resolve*: part8 from
                                              np >= 64 and nsub >= 2 np (PH % 8 == 0), else per sub-query
  resolve_lds    k_resolve<true>              after k_match*: qn > 64, PH <= 8,192, qn * ceil(PH / 64) <= 2,048
  resolve_g      k_resolve<false>             after k_match*: otherwise
  mr_s2          k_match_resolve_s<2,256>     shared steps, np >= 128, nsub >= 4 np, no LDS resolver, descriptor
                                              not in the arguments; "match_resolve" 1, qn <= 64, PH <= 4,096
  mr_s4          k_match_resolve_s<4,256>     the same with 4,096 < PH <= 8,192
  mr_general     k_match_resolve              the same with qn > 64, PH in (8,192, 16,384] or "match_resolve" 2
  gather         k_gather<W>                  SetSize >= 256: min(ceil(SS / 48), ceil(4,096 / nsub)) > 1 ranges
  answer_p5 / p  k_answer_p5 / k_answer_p     after mr_s2 / mr_s4 (query sets expanded): even E <= 256, nsub >= 512,
                                              SS <= 1,024, no gather; "answer_waves" 5 / 6 (0: p5 for E <= 80)
  answer_s       k_answer_s<W,128>            otherwise, where E <= 256, SS <= 1,024 and no gather
  answer_g       k_answer<W>                  E > 256, SS > 1,024 or after k_gather

(k_answer_s<W,256> and <W,512> are selected by PM_ANSWER_NT alone, read once
per process; they are not driven here.)

Each case builds the product and the oracle on one seeded random DB, asserts
the geometry it relies on (ChunkSize, SetSize, PrimaryHintNum, np, qn, nsub),
runs two or more Query calls per client (the later ones after the first one's
refresh), asserts from the counters that exactly the expected forms ran the
expected number of times, and compares every response, success flag, batch
counter and every partition's exported state with the oracle bit for bit
(XORs and indices: the tolerance is zero).  The inputs of every case hold, as
counted from the ids and the oracle's responses alone, a failed sub-query, an
id repeated inside a batch, an id answered in an earlier batch (the local
cache) and a dummy-padded slot, so the resolver's branches run in every form.
"""
import numpy as np
import pytest

from tests.test_gpu_parity import SEED, STATE_KEYS

pytestmark = pytest.mark.gpu

FORMS = ("step", "resolve_lds", "resolve_g", "mr_s2", "mr_s4", "mr_general", "gather",
         "answer_p5", "answer_p", "answer_s", "answer_g")
MATCH = {"match": "host_path_match", "match_part": "host_path_match_part", "match_part8": "host_path_match_part8"}


def form_counts(ctxs):
    """The step-form counters summed over contexts; "nhelp": k_step's helpers (total_ms of "step")."""
    ctxs = ctxs if isinstance(ctxs, (list, tuple)) else [ctxs]
    out = {k: sum(c.timing_get("host_path_" + k)[0] for c in ctxs) for k in FORMS}
    out.update({k: sum(c.timing_get(name)[0] for c in ctxs) for k, name in MATCH.items()})
    out["nhelp"] = sum(int(c.timing_get("host_path_step")[1]) for c in ctxs)
    return out


def assert_forms(ctxs, steps, forms, nhelp=0):
    """Every form of `forms` ran once per step, k_step with nhelp helpers; every sibling counter is 0."""
    want = dict.fromkeys(FORMS + tuple(MATCH) + ("nhelp",), 0)
    for k in forms:
        want[k] = steps
    want["nhelp"] = nhelp * steps
    got = form_counts(ctxs)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}


class Case:
    def __init__(self, name, forms, P, rows, E, F, qn, geom, S=1, fixture="ctx", batches=2, nhelp=0, opts=None, seed=0,
                 ids=None):
        self.name, self.forms, self.P, self.rows, self.E, self.F, self.qn = name, forms, P, rows, E, F, qn
        self.geom, self.S, self.fixture, self.batches, self.nhelp = geom, S, fixture, batches, nhelp
        self.opts, self.seed = opts or {}, seed
        self.ids = ids   # a function (case, db) -> ids [batches, S, n] instead of inputs()' seeded ones (cached per shape)
        self.N, self.n, self.np, self.nsub = P * rows, P * qn, S * P, S * P * qn

    def shape(self):   # what the inputs and the oracle's run depend on
        return (self.P, self.rows, self.E, self.F, self.qn, self.S, self.batches, self.seed,
                self.ids.__name__ if self.ids else None)


    def plan(self):
        """pm.step_plan for this case's steps (host arithmetic; under the options set when it is called): an
        engine's own step for one client, a group's shared step for several."""
        import pacmann_amd as pm
        return pm.step_plan(0 if self.S == 1 else 1, self.np, self.nsub, self.qn, self.geom[2], self.geom[1], self.E,
                            no_fuse=self.fixture == "ctx_unfused")


UNFUSED = ("match", "resolve_g", "answer_s")
# geom: (ChunkSize, SetSize, PrimaryHintNum, np, nsub).  seed: of the ids, chosen (on the CPU, from the oracle's
# run) so that the case holds the four branch conditions of the module docstring.
CASES = [
    # ---- engine_step: one client ----
    # 2 * 8 + 4 = 20 workgroups before the helpers: (240 - 20) / 8 = 27 -> nhelp 3
    Case("step-nhelp3-W2", ("step",), P=4, rows=7500, E=8, F=4, qn=2, geom=(256, 32, 1024, 4, 8), nhelp=3, batches=4, seed=4),
    # 2 * 64 + 32 = 160: (240 - 160) / 64 = 1
    Case("step-nhelp1", ("step",), P=32, rows=500, E=8, F=4, qn=2, geom=(64, 8, 256, 32, 64), nhelp=1),
    # E & ~3 = 260 > 256 gathered words: no helpers; odd E: k_step<1>
    Case("step-nhelp0-W1", ("step",), P=4, rows=500, E=261, F=4, qn=4, geom=(64, 8, 256, 4, 16), nhelp=0, seed=2),
    Case("unfused-W2", UNFUSED, P=4, rows=500, E=8, F=4, qn=4, geom=(64, 8, 256, 4, 16), fixture="ctx_unfused", seed=2),
    Case("unfused-W1", UNFUSED, P=4, rows=500, E=5, F=4, qn=4, geom=(64, 8, 256, 4, 16), fixture="ctx_unfused", seed=2),
    # the staged LDS resolver: qn > 64 and qn * ceil(PH / 64) <= 2,048.  PH 1,792 (28 words): qn 65..73;
    # PH 1,024 (16 words): qn 65..128; the neighbours above take the global-memory form.  nsub > 112: no k_step
    Case("lds-PH1792-qn65", ("match", "resolve_lds", "answer_s"), P=2, rows=5000, E=8, F=8, qn=65,
         geom=(256, 20, 1792, 2, 130), seed=4),
    Case("lds-PH1792-qn73", ("match", "resolve_lds", "answer_s"), P=2, rows=5000, E=8, F=8, qn=73,
         geom=(256, 20, 1792, 2, 146)),
    Case("g-PH1792-qn74", UNFUSED, P=2, rows=5000, E=8, F=8, qn=74, geom=(256, 20, 1792, 2, 148), seed=7),
    Case("lds-PH1024-qn128", ("match", "resolve_lds", "answer_s"), P=2, rows=5000, E=8, F=4, qn=128,
         geom=(256, 20, 1024, 2, 256)),
    Case("g-PH1024-qn129", UNFUSED, P=2, rows=5000, E=8, F=4, qn=129, geom=(256, 20, 1024, 2, 258)),
    # SetSize 296 >= 256: min(ceil(296 / 48), ceil(4,096 / 32)) = 7 gather ranges per sub-query
    Case("gather-W2", ("match", "resolve_g", "gather", "answer_g"), P=2, rows=600000, E=4, F=4, qn=16,
         geom=(2048, 296, 8192, 2, 32), fixture="ctx_unfused"),
    Case("gather-W1", ("match", "resolve_g", "gather", "answer_g"), P=2, rows=600000, E=5, F=4, qn=16,
         geom=(2048, 296, 8192, 2, 32), fixture="ctx_unfused"),
    # E > 256 words: the generic answer kernel, SetSize 16: no gather; odd E: k_answer<1>
    Case("answer_g-W1", ("match", "resolve_g", "answer_g"), P=4, rows=2000, E=257, F=4, qn=4,
         geom=(128, 16, 512, 4, 16), fixture="ctx_unfused"),
    # ---- shared steps: S clients of one server (pm_batchpir_group_query) ----
    Case("part8", ("match_part8", "resolve_g", "answer_s"), S=32, P=2, rows=500, E=8, F=4, qn=2,
         geom=(64, 8, 256, 64, 128)),
    # 4,096 < PH <= 8,192: k_match_resolve_s<4,256>; ChunkSize 1,024 from 65,793 rows per partition
    # (the least with floor(2 sqrt(rows)) > 512)
    Case("mr_s4-p5-512", ("mr_s4", "answer_p5"), S=64, P=2, rows=65793, E=4, F=5, qn=4,
         geom=(1024, 68, 5120, 128, 512), opts={"answer_waves": 5}, seed=1),
    Case("mr_s4-p-512", ("mr_s4", "answer_p"), S=64, P=2, rows=65793, E=4, F=5, qn=4,
         geom=(1024, 68, 5120, 128, 512), opts={"answer_waves": 6}, seed=1),
    # 645 = 129 * 5 sub-queries: the pair form's last workgroup holds one sub-query alone
    Case("mr_s4-p5-645", ("mr_s4", "answer_p5"), S=43, P=3, rows=65793, E=4, F=8, qn=5,
         geom=(1024, 68, 7168, 129, 645), opts={"answer_waves": 5}),
    Case("mr_s4-p-645", ("mr_s4", "answer_p"), S=43, P=3, rows=65793, E=4, F=8, qn=5,
         geom=(1024, 68, 7168, 129, 645), opts={"answer_waves": 6}),
    # odd E: no pair form
    Case("mr_s4-answer_s", ("mr_s4", "answer_s"), S=64, P=2, rows=65793, E=5, F=5, qn=4,
         geom=(1024, 68, 5120, 128, 512), seed=1),
    # qn 74 at PH 1,792: above the LDS resolver's window and above the small form's 64 sub-queries per partition
    Case("mr_general-qn74", ("mr_general", "answer_s"), S=64, P=2, rows=5000, E=8, F=8, qn=74,
         geom=(256, 20, 1792, 128, 9472)),
    # the least shape of the k_match_resolve_s chain (512 = 128 * 4), by both forms: test_match_resolve_general_...
    Case("mr_s2-512", ("mr_s2", "answer_p5"), S=64, P=2, rows=2500, E=8, F=4, qn=4,
         geom=(128, 20, 512, 128, 512), opts={"match_resolve": 1, "answer_waves": 5}),
    Case("mr_general-512", ("mr_general", "answer_s"), S=64, P=2, rows=2500, E=8, F=4, qn=4,
         geom=(128, 20, 512, 128, 512), opts={"match_resolve": 2}),
]
BY_NAME = {c.name: c for c in CASES}
PAIR = ("mr_s2-512", "mr_general-512")   # run together by test_match_resolve_general_equals_small


_built_ids = {}


def inputs(case):
    """The DB, the ids [batches, S, n] and the clients' seeds.  Planted: position 3 repeats position 1 inside
    every batch, and positions 0 and 2 of every later batch repeat the first batch's (the local cache)."""
    db = np.random.default_rng(1000 * case.rows + case.E).integers(0, 2**64, size=case.N * case.E, dtype=np.uint64)
    if case.ids:
        if case.shape() not in _built_ids:
            _built_ids[case.shape()] = case.ids(case, db)
            _built_ids[case.shape()].setflags(write=False)
        return db, _built_ids[case.shape()], [SEED + 31 * i for i in range(case.S)]
    rng = np.random.default_rng([case.seed, case.rows, case.n, case.S])
    ids = rng.integers(0, case.N, size=(case.batches, case.S, case.n), dtype=np.uint64)
    ids[:, :, 3] = ids[:, :, 1]
    ids[1:, :, 0] = ids[0, :, 0]
    ids[1:, :, 2] = ids[0, :, 2]
    return db, ids, [SEED + 31 * i for i in range(case.S)]


def branch_counts(case, ids, want):
    """From the ids and the oracle's responses alone: sub-queries that failed (a kept id with an all-zero
    response: the DB rows are random), ids repeated among a batch's kept ones, kept ids answered in an earlier
    batch of their client, and dummy-padded slots.  Kept: among the first qn ids of its partition in the batch
    (batch-pir.go:195-200 drops the rest)."""
    out = dict(failed=0, repeated=0, cached=0, dummy=0)
    for i in range(case.S):
        answered = set()
        for b in range(case.batches):
            q = ids[b, i].astype(np.int64)
            part = q // case.rows
            seen = np.zeros(case.P, dtype=np.int64)
            kept = {}
            nkept = 0
            for pos, (x, p) in enumerate(zip(q.tolist(), part.tolist())):
                if seen[p] < case.qn:
                    nkept += 1
                    kept[x] = bool(want[b, i, pos].any())
                seen[p] += 1
            out["dummy"] += int(np.maximum(case.qn - seen, 0).sum())
            out["repeated"] += nkept - len(kept)
            out["failed"] += sum(not ok for ok in kept.values())
            out["cached"] += sum(x in answered for x in kept)
            answered |= {x for x, ok in kept.items() if ok}
    return out


_reference = {}
_before = {}


def oracle_run(oracle, case):
    """Every client's responses per batch, its counters and every partition's Config and state after the last
    batch: computed once per shape, shared by the cases of that shape, read-only."""
    key = case.shape()
    if key not in _reference:
        db, ids, seeds = inputs(case)
        ors = [oracle.SimpleBatchPianoPIR(case.N, case.E * 8, 2 * case.P, db, case.F, seed=sd) for sd in seeds]
        for o in ors:
            o.Preprocessing()
        keep = case.S == 1 and case.forms == ("step",)   # k_step's cases: every partition's state before each batch too
        before, want = [], []
        for b in range(case.batches):
            if keep:
                before.append([ors[0].sub(p).export_state() for p in range(case.P)])
            want.append(np.stack([o.Query(ids[b, i])[0] for i, o in enumerate(ors)]))
        want = np.stack(want)
        state = [[o.sub(p).export_state() for p in range(case.P)] for o in ors]
        cfg = [ors[0].sub(p).Config() for p in range(case.P)]
        stats = [o.stats() for o in ors]
        for a in (want, *[x[k] for st in state for x in st for k in STATE_KEYS]):
            a.setflags(write=False)
        _reference[key] = (want, state, stats, cfg)
        _before[key] = before
    return _reference[key]


def oracle_before(oracle, case):
    """Of a one-client k_step case: per batch, every partition's exported state before it (the same oracle run)."""
    oracle_run(oracle, case)
    assert case.S == 1 and case.forms == ("step",)
    return _before[case.shape()]


def run_case(case, request, oracle, step_hook=None):
    """Runs `case` on the product with every assertion of the module docstring; returns what it answered.
    step_hook(server), if given, is called after every batch (one step); its results are returned as well."""
    import pacmann_amd as pm
    ctx = request.getfixturevalue(case.fixture)
    db, ids, seeds = inputs(case)
    want, state, stats, ocfg = oracle_run(oracle, case)
    got_branches = branch_counts(case, ids, want)
    assert all(got_branches.values()), got_branches
    E, EX = case.E, case.E & ~3
    rows = db.reshape(case.N, E)
    try:
        for k, v in case.opts.items():
            pm.set_option(k, v)
        server = pm.SimpleBatchPianoPIR(case.N, E * 8, 2 * case.P, db, case.F, seed=seeds[0], ctx=ctx)
        clients = [server] + [server.Client(sd) for sd in seeds[1:]]
        # the geometry the expected forms follow from
        assert server.Config()["PartitionNum"] == case.P and server.Config()["PartitionSize"] == case.rows
        for p in range(case.P):
            c = server.SubConfig(p)
            assert (c["ChunkSize"], c["SetSize"], c["PrimaryHintNum"]) == case.geom[:3], (p, c)
            assert c["PrimaryHintNum"] % 8 == 0
            assert c["MaxQueryNum"] > case.batches * case.qn   # no partition reaches its budget: one step per call
            for k in ("DBSize", "ChunkSize", "SetSize", "MaxQueryNum", "PrimaryHintNum", "MaxQueryPerChunk"):
                assert c[k] == ocfg[p][k], (p, k)
        assert (case.np, case.nsub) == case.geom[3:] and case.n // case.P == case.qn
        for c in clients:
            c.Preprocessing()
        grp = pm.BatchPIRGroup(clients) if case.S > 1 else None
        ctx.timing_reset()
        answers, hooked = [], []
        for b in range(case.batches):
            got, ok = grp.QueryWithMask(ids[b]) if grp else (x[None] for x in server.QueryWithMask(ids[b, 0]))
            answers.append((got, ok))
            if step_hook:
                hooked.append(step_hook(server))
            assert np.array_equal(got, want[b]), b
            for i in range(case.S):
                r = rows[ids[b, i].astype(np.int64)]
                assert np.array_equal(got[i][ok[i]][:, :EX], r[ok[i]][:, :EX]), (b, i)
                assert not got[i][:, EX:].any(), (b, i)   # the words past E & ~3 stay out of the XOR
                assert not got[i][~ok[i]].any(), (b, i)
        assert_forms(ctx, case.batches, case.forms, case.nhelp)
        plan, counted = case.plan(), form_counts(ctx)   # the selector's own answer for the shape, without a launch
        assert set(plan["forms"]) == {k for k in FORMS + tuple(MATCH) if counted[k]}, (plan["forms"], counted)
        assert plan["nhelp"] * case.batches == counted["nhelp"]
        states = []
        for i, c in enumerate(clients):
            for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
                assert c.stats()[key] == stats[i][key], (i, key)
            assert c.stats()["PrepCount"] == 1
            for p in range(case.P):
                a = c.export_state(p)
                for k in STATE_KEYS:
                    assert np.array_equal(a[k], state[i][p][k]), (i, p, k)
                states.append(a)
        return (answers, states, hooked) if step_hook else (answers, states)
    finally:
        for k in case.opts:
            pm.set_option(k, -2)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.name not in PAIR])
def test_step_form(request, oracle, name):
    run_case(BY_NAME[name], request, oracle)


def test_match_resolve_general_equals_small(request, oracle):
    """ "match_resolve" 2 sends the 512-sub-query chain shape through the general k_match_resolve and k_answer_s
    instead of k_match_resolve_s<2,256> and k_answer_p5: the same responses, flags and client states."""
    (a1, s1), (a2, s2) = (run_case(BY_NAME[n], request, oracle) for n in PAIR)
    for (g1, ok1), (g2, ok2) in zip(a1, a2):
        assert np.array_equal(g1, g2) and np.array_equal(ok1, ok2)
    for x, y in zip(s1, s2):
        for k in STATE_KEYS:
            assert np.array_equal(x[k], y[k]), k


def test_every_form_has_a_case():
    reached = {f for c in CASES for f in c.forms}
    assert reached == set(FORMS) | {"match", "match_part8"}   # k_match_part: test_batch_pir_group_hint_search_paths
    assert {c.nhelp for c in CASES if c.forms == ("step",)} == {0, 1, 3}

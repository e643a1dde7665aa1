"""k_step's speculation, path by path: kept, redone and refused-helper answers against the oracle.

k_step (pm_query.hip) answers before the resolution is known: an answer workgroup guesses its sub-query's
resolution (step_guess), gathers the first 1 / (nhelp + 1) of the guessed set, merges the partial XORs of up to
three helper workgroups (helper_role) if each of them guessed the same (help_ok), and then either keeps that work
(kept and help_ok) or gathers the whole set again for the resolver's record (redo).  The bits that come out are the
same on every path, so these tests read the path from the speculation record (pm_batchpir_step_spec, contexts
created with PM_STEP_SPEC=1: one word per sub-query, include/pacmann.h) and force the paths that otherwise depend on
timing: "step_help" 0 / 2 changes the helpers per sub-query, "step_help_spoil" makes chosen helpers publish a guess
no answer accepts (the refused-helper path, for dummy and real sub-queries), PM_NO_GUESS=1 makes every answer wait.

Every variant runs test_gpu_step_forms.run_case: every response, success flag, batch counter and every partition's
exported state equal the oracle's bit for bit, the counted forms and helpers equal step_plan's.  One oracle run per
shape serves all its variants.

The record is checked against a host model of the step (model_step below), computed from the oracle's state before
each batch and the oracle's PRF alone: the guess from the state at the start of the step, the resolution by the
sequential Client.Query rule (oracle/pm_oracle.cpp client_query, pir.go:354-471).  The model's own success flags
are checked against the oracle's responses.  What the code fixes regardless of timing is asserted per sub-query
(redo == !kept || !help_ok; helped == nhelp > 0 and a guess; kept implies gmode == mode; the resolution's mode
equals the model's); (gmode, mode, kept) as the set of combinations a case reaches, which equals the model's.

Reachable (gmode, mode, kept), from step_guess (pm_query.hip:1891-1939), answer_mode (:1801-1805) and the
resolver's chain (:1245-1337); "none": no guess (record value 7):

  gmode  mode     kept  how
  dummy  dummy    yes   SUB_DUMMY: step_guess :1897, resolver :1248; the only combination of a dummy
  final  final    yes   the first stale candidate and the predicted in-chunk index hold
  final  final    no    an earlier sub-query of the step took the candidate hint (the resolver moves on, :1275-1284),
                        or an earlier one of the same chunk failed (the in-chunk index is lower than predicted)
  final  chained  no    a hint refreshed earlier in the step is now the first match (:1286-1315, flags bit 0)
  final  zero     no    an id repeated in its batch after a success (ST_DUP, :1255-1261), or no hint left
  none   zero     no    no candidate (ST_ENOHIT, :1306) or a full chunk (:1271)
  none   cached   no    an id answered in an earlier batch is SUB_HOSTCACHE (pm_engine.cpp add_sub), for which
                        step_guess makes no guess (:1901): a cached id is never guessed final
  none   chained  no    no candidate at the start of the step, but a hint refreshed earlier in it matches
  none   final    no    the predicted in-chunk index reaches MaxQueryPerChunk while an earlier sub-query of the chunk
                        failed: a chunk one query short of full, planted by spec-fullchunk (full_chunk_ids)
  PM_NO_GUESS=1: none with every mode.

Unreachable, and asserted never to appear: any kept combination but the two above; dummy with another mode; a
guess of final resolved cached or dummy; a guess other than final / dummy / none.
"""
import os

import numpy as np
import pytest

from tests.test_gpu_parity import SEED
from tests.test_gpu_step_forms import BY_NAME, Case, inputs, oracle_before, oracle_run, run_case

pytestmark = pytest.mark.gpu

ZERO, FINAL, CHAINED, CACHED, DUMMY, NONE = 0, 1, 2, 3, 4, 7   # answer modes (pm_query.hip:1729); NONE: no guess
DEFAULT_PP = 0x7FFFFFFF

# (gmode, mode, kept) the default variants reach between them (the table above)
REACHED = {(DUMMY, DUMMY, True), (FINAL, FINAL, True), (FINAL, FINAL, False), (FINAL, CHAINED, False),
           (FINAL, ZERO, False), (NONE, ZERO, False), (NONE, CACHED, False), (NONE, CHAINED, False), (NONE, FINAL, False)}
NO_GUESS = {(NONE, m, False) for m in (ZERO, FINAL, CHAINED, CACHED, DUMMY)}

def _ctx_with(env):
    import pacmann_amd as pm
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pm.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctx_spec():
    """A context whose k_step keeps its speculation record (PM_STEP_SPEC=1, read at context creation)."""
    return _ctx_with({"PM_STEP_SPEC": "1"})


@pytest.fixture(scope="module")
def ctx_spec_noguess():
    """The same with PM_NO_GUESS=1: no answer starts before its resolution."""
    return _ctx_with({"PM_STEP_SPEC": "1", "PM_NO_GUESS": "1"})


def first_hint(oracle, rk, tags, pps, CS, chunk, off):
    """The first primary hint whose set holds (chunk, off): client_query's search (pir.go:403-419)."""
    ho = oracle.prf_batch(rk, tags, np.full(len(tags), chunk, dtype=np.uint64)) & np.uint64(CS - 1)
    m = (ho == off) & ((pps == DEFAULT_PP) | (pps // np.uint64(CS) != chunk))
    return int(np.flatnonzero(m)[0]) if m.any() else None


def full_chunk_ids(case, db):
    """Ids that plant (no guess, final): driven by the oracle's own state on the CPU, partition 0's chunk
    `case.seed % (SetSize - 1)` is filled to MaxQueryPerChunk - 1 successes over the first batches (fresh ids of the
    chunk that have a hint, the partition's last qn positions of each batch); the last batch then sends two fresh ids
    of that chunk, the first without a hint.  It fails, so the second's predicted in-chunk index is MaxQueryPerChunk
    (no guess, step_guess :1934) while the resolver finds the chunk one short of full and answers it.  The other
    positions hold ids of the other partitions with inputs()' plants: position 3 repeats position 1, positions 0
    and 2 of every later batch repeat the first batch's."""
    from oracle import oracle as O
    o = O.SimpleBatchPianoPIR(case.N, case.E * 8, 2 * case.P, db, case.F, seed=SEED)
    o.Preprocessing()
    c = o.sub(0).Config()
    CS, Qpc, qn = c["ChunkSize"], c["MaxQueryPerChunk"], case.qn
    chunk = case.seed % (c["SetSize"] - 1)
    rng = np.random.default_rng([case.seed, case.rows, case.n, 7])
    unused = list(range(chunk * CS, (chunk + 1) * CS))
    ids = np.zeros((case.batches, 1, case.n), dtype=np.uint64)
    for b in range(case.batches):
        row = rng.integers(case.rows, case.N, size=case.n, dtype=np.uint64)
        if b:
            row[0], row[2] = ids[0, 0, 0], ids[0, 0, 2]
        row[3] = row[1]
        st = o.sub(0).export_state()
        hinted = [x for x in unused if first_hint(O, st["round_keys"], st["primary_tag"], st["primary_pp"], CS, chunk,
                                                  x % CS) is not None]
        done = int(st["hist"][chunk])
        if b < case.batches - 1:
            mine = hinted[:min(qn, Qpc - 1 - done)]
        else:
            bare = [x for x in unused if x not in hinted]
            assert done == Qpc - 1 and bare and hinted, (case.seed, done, len(bare), len(hinted))
            mine = [bare[0], hinted[0]]
        unused = [x for x in unused if x not in mine]
        row[case.n - len(mine):] = mine   # partition 0 holds the ids below `rows`: local = global
        ids[b, 0] = row
        o.Query(row)
    return ids


def model_step(oracle, case, cfg, before, ids_b, answered):
    """The model of one step (one batch of one client): per sub-query in the product's order (partition-major, qn
    slots per partition: the partition's first qn ids, then dummies) its (gmode, mode, kept) and whether it
    succeeds.  before[p]: the oracle's exported state of partition p before the batch; answered: the ids that
    succeeded in earlier batches (the host's localCache)."""
    out = []
    q = ids_b.astype(np.int64)
    for p in range(case.P):
        c, st = cfg[p], before[p]
        CS, Qpc, mask = c["ChunkSize"], c["MaxQueryPerChunk"], c["ChunkSize"] - 1
        rk = st["round_keys"]
        tag0, pp0, hist0 = st["primary_tag"], st["primary_pp"], st["hist"]
        tag, pp, hist = tag0.copy(), pp0.copy(), hist0.copy()

        def first_match(tags, pps, chunk, off):
            return first_hint(oracle, rk, tags, pps, CS, chunk, off)
        mine = [int(x) - p * case.rows for x in q.tolist() if x // case.rows == p][:case.qn]
        subs = [("cached" if x + p * case.rows in answered else "real", x) for x in mine]
        subs += [("dummy", 0)] * (case.qn - len(subs))
        refreshed, ok_ids = set(), set()
        for j, (kind, x) in enumerate(subs):
            if kind == "dummy":
                out.append((DUMMY, DUMMY, True, False, None))
                continue
            if kind == "cached":
                out.append((NONE, CACHED, False, True, x + p * case.rows))
                continue
            chunk, off = x // CS, x % CS
            # the guess: the state at the start of the step (step_guess; predict_ing's in-chunk index)
            real_before = [y for k, y in subs[:j] if k == "real"]
            firsts = [y for i, y in enumerate(real_before) if y not in real_before[:i]]
            sg = int(hist0[chunk]) + sum(y // CS == chunk for y in firsts)
            c1 = first_match(tag0, pp0, chunk, off)
            g = (c1, chunk, sg, int(tag0[c1]), int(pp0[c1])) if c1 is not None and sg < Qpc else None
            gmode = FINAL if g else NONE
            # the resolution: Client.Query in order, over the hints as refreshed so far in this step
            mode, r = ZERO, None
            if x not in ok_ids and hist[chunk] < Qpc:
                hit = first_match(tag, pp, chunk, off)
                if hit is not None:
                    ing = int(hist[chunk])
                    mode, r = (CHAINED if hit in refreshed else FINAL), (hit, chunk, ing, int(tag[hit]), int(pp[hit]))
                    tag[hit], pp[hit] = st["backup_tag"][chunk * Qpc + ing], x
                    hist[chunk] += 1
                    refreshed.add(hit)
                    ok_ids.add(x)
            ok = mode != ZERO or x in ok_ids   # a repeated id is answered from its first occurrence
            out.append((gmode, mode, gmode == mode and g == r, ok, x + p * case.rows))
    return out


FULLCHUNK_SEED = 0
# geom: (ChunkSize, SetSize, PrimaryHintNum, np, nsub), worked out with the oracle's Config on the CPU; seed: of
# the ids, chosen on the CPU from the oracle's run and model_step (branch_counts' four conditions in every shape)
SHAPES = [
    BY_NAME["step-nhelp3-W2"],   # SetSize 32, ChunkSize 256: chunks 30, 31 lie past the 7,500 rows (the last helper's range)
    BY_NAME["step-nhelp1"],
    BY_NAME["step-nhelp0-W1"],
    Case("spec-E80", ("step",), P=4, rows=7500, E=80, F=4, qn=2, geom=(256, 32, 1024, 4, 8), nhelp=3, batches=4, seed=4),
    # odd E, E & ~3 = 256 = kHelpWords: one partial word per thread up to the limit
    Case("spec-E259-W1", ("step",), P=4, rows=500, E=259, F=4, qn=2, geom=(64, 8, 256, 4, 8), nhelp=3, batches=4, seed=4),
    # 2 * 72 + 24 + 72 = 240 workgroups with one helper each: the most a launch with helpers has
    Case("spec-grid240", ("step",), P=24, rows=500, E=8, F=4, qn=3, geom=(64, 8, 256, 24, 72), nhelp=1, batches=4, seed=0),
    # 2 * 112 + 28 = 252 >= 240: no helpers
    Case("spec-grid252", ("step",), P=28, rows=500, E=8, F=4, qn=4, geom=(64, 8, 256, 28, 112), nhelp=0, batches=2, seed=0),
    # the least SetSize (a multiple of 4) with three helpers: every range is one chunk, and chunk 3 (rows 48-63)
    # lies past the partition's 40 rows
    Case("spec-SS4", ("step",), P=4, rows=40, E=8, F=4, qn=2, geom=(16, 4, 64, 4, 8), nhelp=3, batches=4, seed=0),
    # a chunk filled to MaxQueryPerChunk - 1 = 55 over eight batches, then the pair of full_chunk_ids: (none, final).
    # 2 * 32 + 4 = 68 workgroups: nhelp 3; 9 * 8 = 72 queries < MaxQueryNum 138
    Case("spec-fullchunk", ("step",), P=4, rows=500, E=8, F=4, qn=8, geom=(64, 8, 256, 4, 32), nhelp=3, batches=9,
         seed=FULLCHUNK_SEED, ids=full_chunk_ids),
]
SHAPE = {c.name: c for c in SHAPES}


def variants(c):
    """(variant name, options, fixture, expected nhelp) of shape c."""
    out = [("default", {}, "ctx_spec", c.nhelp), ("noguess", {}, "ctx_spec_noguess", c.nhelp)]
    if c.nhelp:
        out.append(("help0", {"step_help": 0}, "ctx_spec", 0))
        out += [("spoil%d" % m, {"step_help_spoil": m}, "ctx_spec", c.nhelp) for m in (1, 2, 4, 7)]
    if c.nhelp == 3:
        out.append(("help2", {"step_help": 2}, "ctx_spec", 2))
        out.append(("help2-spoil7", {"step_help": 2, "step_help_spoil": 7}, "ctx_spec", 2))
    return out


VARIANTS = [(c.name, *v) for c in SHAPES for v in variants(c)]


_model = {}


def reference(oracle, case):
    """The model of every step of the shape, from the shape's one oracle run (test_gpu_step_forms.oracle_run, which
    keeps every partition's state before each batch): once per shape, shared by its variants."""
    key = case.shape()
    if key not in _model:
        db, ids, seeds = inputs(case)
        want, _, _, cfg = oracle_run(oracle, case)
        steps, answered = [], set()
        for b, before in enumerate(oracle_before(oracle, case)):
            m = model_step(oracle, case, cfg, before, ids[b, 0], answered)
            answered |= {gid for (_, mode, _, ok, gid) in m if ok and gid is not None}
            # the model against the oracle: an id succeeds in the model iff the oracle answered it
            okm = {gid: ok for (_, _, _, ok, gid) in m if gid is not None}
            for pos, gid in enumerate(ids[b, 0].astype(np.int64).tolist()):
                if gid in okm:
                    assert okm[gid] == bool(want[b, 0, pos].any()), (case.name, b, pos)
            steps.append(m)
        _model[key] = steps
    return _model[key]


def fields(w):
    import pacmann_amd as pm
    return pm.step_spec_fields(w)


_seen = {}   # (shape, variant) -> the (gmode, mode, kept) combinations its record held


def run_variant(request, oracle, shape, variant, opts, fixture, nhelp):
    import pacmann_amd as pm
    base = SHAPE[shape]
    model = reference(oracle, base)
    case = Case(base.name, base.forms, P=base.P, rows=base.rows, E=base.E, F=base.F, qn=base.qn, geom=base.geom,
                fixture=fixture, batches=base.batches, nhelp=nhelp, opts=opts, seed=base.seed, ids=base.ids)
    try:
        for k, v in opts.items():
            pm.set_option(k, v)
        assert case.plan()["nhelp"] == nhelp   # what the options make of the shape, before anything runs
    finally:
        for k in opts:
            pm.set_option(k, -2)
    _, _, records = run_case(case, request, oracle, step_hook=lambda server: server.step_spec())
    spoil = opts.get("step_help_spoil", 0) & ((1 << nhelp) - 1)   # the bits of helpers that exist
    seen, refused, spoiled_modes = set(), 0, set()
    for b, (rec, m) in enumerate(zip(records, model)):
        assert len(rec) == case.nsub == len(m)
        for s, (w, (gmode, mode, kept, _, _)) in enumerate(zip(rec.tolist(), m)):
            f = fields(w)
            at = (b, s, f)
            assert f["written"], at
            assert f["redo"] == (not f["kept"] or not f["help_ok"]), at
            assert f["helped"] == (nhelp > 0 and f["gmode"] in (DUMMY, FINAL)), at
            assert f["gmode"] in (DUMMY, FINAL, NONE), at
            assert not f["kept"] or f["gmode"] == f["mode"], at
            assert f["help_ok"] or f["helped"], at
            assert f["mode"] == mode, (at, mode)   # the resolution does not depend on timing
            if mode == DUMMY:
                assert (f["gmode"], f["kept"]) == ((NONE, False) if fixture == "ctx_spec_noguess" else (DUMMY, True)), at
            if fixture == "ctx_spec_noguess":
                assert f["gmode"] == NONE and f["redo"] and not f["kept"] and not f["helped"], at
            if spoil and f["helped"]:
                assert not f["help_ok"] and f["redo"], at
                spoiled_modes.add(f["gmode"])
            refused += f["helped"] and not f["help_ok"]
            seen.add((f["gmode"], f["mode"], f["kept"]))
    print("%s-%s: %d helped answers refused their helpers; combinations %s" % (shape, variant, refused, sorted(seen)))
    if spoil:
        assert spoiled_modes == {FINAL, DUMMY}
    if fixture == "ctx_spec_noguess":
        assert seen <= NO_GUESS
    else:
        # the guesses too, as a set: those of the model (the state before the step decides them)
        assert seen == {(g, mo, k) for step in model for (g, mo, k, _, _) in step}, shape
    _seen[(shape, variant)] = seen
    return seen


@pytest.mark.parametrize("shape,variant,opts,fixture,nhelp", VARIANTS, ids=["%s-%s" % v[:2] for v in VARIANTS])
def test_step_spec(request, oracle, shape, variant, opts, fixture, nhelp):
    run_variant(request, oracle, shape, variant, opts, fixture, nhelp)


def test_step_spec_errors(ctx, ctx_spec):
    """pm_batchpir_step_spec where there is no record: a context without PM_STEP_SPEC=1; a context with it before
    any step, and after a step that the three kernels ran (PM_NO_FUSE=1), whose record buffer k_step never filled."""
    import pacmann_amd as pm
    c = SHAPE["spec-SS4"]
    db, ids, seeds = inputs(c)

    def server(cx):
        s = pm.SimpleBatchPianoPIR(c.N, c.E * 8, 2 * c.P, db, c.F, seed=seeds[0], ctx=cx)
        s.Preprocessing()
        return s
    s = server(ctx)
    s.Query(ids[0, 0])
    with pytest.raises(RuntimeError, match=": no speculation record: the context was created without PM_STEP_SPEC=1$"):
        s.step_spec()
    s = server(ctx_spec)
    with pytest.raises(RuntimeError, match=": no speculation record: the last step did not run k_step$"):
        s.step_spec()
    s.Query(ids[0, 0])
    assert len(s.step_spec()) == c.nsub
    cx = _ctx_with({"PM_STEP_SPEC": "1", "PM_NO_FUSE": "1"})
    s = server(cx)
    s.Query(ids[0, 0])
    assert cx.timing_get("host_path_step")[0] == 0 and cx.timing_get("host_path_answer_s")[0] == 1
    with pytest.raises(RuntimeError, match=": no speculation record: the last step did not run k_step$"):
        s.step_spec()


def test_step_spec_combinations(request, oracle):
    """The default variants between them reach every combination of the table, and no variant shows one the table
    calls unreachable.  Variants that have not run in this process (a selection of tests) run here."""
    for v in VARIANTS:
        if (v[0], v[1]) not in _seen:
            run_variant(request, oracle, *v)
    default = set().union(*[s for (_, variant), s in _seen.items() if variant == "default"])
    assert default == REACHED, (sorted(default - REACHED), sorted(REACHED - default))
    guessing = set().union(*[s for (_, variant), s in _seen.items() if variant != "noguess"])
    assert guessing <= REACHED, sorted(guessing - REACHED)
    assert set().union(*[s for (_, variant), s in _seen.items() if variant == "noguess"]) <= NO_GUESS

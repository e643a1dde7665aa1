"""The cases that drive every branch of the device loop's team round (k_team_round of pm_drl.hip, the helpers of
pm_search_dev.h, the gate drl_plan of pm_devloop.cpp), with the oracle's evidence that each one reaches its branch.

Only the oracle executes Go's exact order, so only it can say whether a case popped from an empty heap, dropped an
id in the bucketing or compared two equal distances: oracle.Graph.trace() counts those events beside its own run
(or_trace in pm_oracle.h).  tests/test_devloop_cases.py asserts every case's counters without a GPU;
tests/test_gpu_devloop_rounds.py runs the same cases through the device loop and the host loop.

BatchSize is m, so P = m / 2 partitions and queryNumToMake qn = 2 * parallel; a round fetches parallel * m ids.
The vertex counts are the smallest at which the call stays inside every partition's budget (step * qn below
MaxQueryNum = floor(sqrt(PS) ln PS): 54, 88, 141, 221, 345 at PartitionSize 128 ... 2,048), so that the gate's
shape limits alone decide the gate cases.
"""
import math
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name dim m parallel step k n graph lone rows S q ngroups gate expect")

GT0 = (">", 0)   # an expected trace count: (">", x), or the exact value
SIFT, TIED = "sift", "tied"


def _c(name, dim, m, parallel, step, k, n, graph, lone=0, rows=SIFT, S=2, q=2, ngroups=1, gate=(), **expect):
    return Case(name, dim, m, parallel, step, k, n, graph, lone, rows, S, q, ngroups, frozenset(gate), expect)


SOME = "0 < succ < total"   # successQueryNum: some entries equal the true neighbour list, some do not

# graph: (generator of tests/datagen.py, its parameters after (n, m)); lone: lone_id_lists(graph, lone).
# gate: the limits of drl_plan the shape is past (empty: the device loop serves the call).
# expect: trace counters summed over the case's sessions, and "succ" (counts()'s successQueryNum: xorSlices XORs
# E & ~3 words, so where E % 4 != 0 every list's tail is zero and succ is 0).
CASES = [
    # scalar decode: m / 4 = 6 is no power of two; a window of 24 crowds one or two of the 12 partitions.
    # E = 62 words: the last 4 neighbours of every list are cut, no entry equals the true list
    _c("scalar-m24", 100, 24, 3, 8, 10, 6144, ("windowed_graph", 24), S=3, q=3, succ=0,
       dropped_ids=GT0, batch_dups=GT0, batch_triples=GT0, skipped_known=GT0, cache_hits=GT0, skipped_zero=GT0),
    # the same decode with whole lists (E = 64): the compare with the true list matches for the answered ids
    _c("scalar-m24-whole", 104, 24, 3, 8, 10, 6144, ("windowed_graph", 24), S=3, q=3, succ=SOME,
       dropped_ids=GT0, batch_dups=GT0, batch_triples=GT0, skipped_known=GT0, cache_hits=GT0),
    # scalar decode: E = (102 + 32) / 2 = 67 words is odd (rows 8-B aligned only); the last 6 neighbours are cut
    _c("scalar-dim102", 102, 32, 3, 6, 10, 8192, ("random_graph",), max_new=GT0, succ=0),
    # scalar decode for dim % 4 != 0 and m % 4 != 0 with whole lists: E = (102 + 26) / 2 = 64, 13 partitions
    _c("scalar-dim102-m26", 102, 26, 3, 6, 10, 6656, ("random_graph",), max_new=GT0, succ=SOME),
    # vector decode, one 16-B chunk per list (no shuffle), parallel 8.  dim 60: E = 32 words; at dim 64 (E = 34)
    # xorSlices leaves the entry's last two words, the whole list, out of every answer and no vertex is ever added
    _c("vec-m4", 60, 4, 8, 10, 5, 2048, ("windowed_graph", 4), S=3,
       batch_dups=GT0, batch_triples=GT0, skipped_known=GT0, succ=SOME),
    # 2, 4 and 16 chunks per list, their flags ORed across the list's lanes: every eighth vertex's list is zero but
    # for one id in a random column (lone_id_lists), so a lane left out of the OR loses a vertex or a success
    _c("vec-m8", 64, 8, 3, 8, 10, 2048, ("windowed_graph", 8), lone=8, S=3, q=3,
       batch_dups=GT0, skipped_known=GT0, partial_zero_lists=GT0, succ=SOME),
    _c("vec-m16", 64, 16, 3, 8, 10, 4096, ("windowed_graph", 16), lone=8, S=3, q=3,
       batch_dups=GT0, skipped_known=GT0, partial_zero_lists=GT0, succ=SOME),
    # n * cpp = 2,048 decode items (two passes of 1,024); P = 32 partitions
    _c("vec-m64", 64, 64, 2, 6, 10, 8192, ("vertex0_graph",), max_new=GT0, partial_zero_lists=GT0, succ=SOME),
    # n = 256 = the workgroup: every lane holds a position; more than 64 new vertices in a round (path_push passes)
    _c("n256-random", 128, 32, 8, 7, 10, 8192, ("random_graph",), max_new=(">", 64), succ=SOME),
    _c("n256-windowed", 128, 32, 8, 7, 10, 8192, ("windowed_graph", 32),
       dropped_ids=GT0, batch_dups=GT0, skipped_known=GT0, skipped_zero=GT0),
    _c("par1", 128, 32, 1, 12, 10, 4096, ("windowed_graph", 32), S=3, q=3, skipped_known=GT0, cache_hits=GT0),
    # one vertex in sixteen has a list: the heap runs dry and refills from the id stream (at one in eight
    # the nine queries hold a single round with both heap pops and stream pops; here five)
    _c("dry-heap", 128, 32, 3, 10, 10, 8192, ("sparse_graph", 0.0625), S=3, q=3,
       stream_pops=GT0, mixed_rounds=GT0, skipped_zero=GT0),
    # no vertex has a list: only the 3 start vertices are ever known, 7 of 10 answer slots are -1
    _c("no-lists", 128, 32, 3, 4, 10, 4096, ("sparse_graph", 0.0), S=2, q=2,
       stream_pops=GT0, padded=2 * 2 * 7, max_new=0, zero_id_positions=GT0, dropped_ids=GT0),
    # 64 prototypes with entries 0..3: equal distances at the start sort, in the heap and in the answer
    _c("ties", 16, 32, 3, 8, 20, 8192, ("windowed_graph", 32), rows=TIED, S=3, q=3,
       tie_pushes=GT0, tie_pops=GT0, start_ties=GT0, answer_ties=GT0),
    _c("vertex0", 128, 32, 3, 6, 10, 8192, ("vertex0_graph",), S=3, q=3, zero_id_positions=GT0, partial_zero_lists=GT0),
    # 5 sessions in 2 teams: 2 + 3
    _c("uneven-teams", 128, 32, 3, 6, 10, 8192, ("random_graph",), S=5, ngroups=2, max_new=GT0),
    # a start set smaller than parallel (BEGIN's A.ns < parallel): 63 vertices give floor(sqrt(63)) = 7 start
    # vertices for 8 pops, so the first round's last pop already draws from the id stream.  PartitionSize 32 and
    # 31: MaxQueryNum 19 against one round of qn = 16
    _c("few-starts", 60, 4, 8, 1, 5, 63, ("windowed_graph", 4), S=3, q=3, short_starts=9, stream_pops=GT0,
       mixed_rounds=GT0),
    # BEGIN, one round, END
    _c("step1", 128, 32, 3, 1, 10, 4096, ("random_graph",), S=2, q=3, max_new=GT0),
    # ---- the gate's limits: the host loop serves these calls ----
    _c("gate-par9", 128, 32, 9, 4, 10, 8192, ("random_graph",), gate=("parallel", "n", "nm")),
    _c("gate-nm", 64, 64, 3, 4, 10, 8192, ("random_graph",), gate=("nm",)),
    # kcap = pow2(8 + 15 * 256) = 4,096: 32,768 + 32,768 + 9,216 = 74,752 B of LDS (step 7: 2,048, 58,368 B, n256)
    _c("gate-lds", 128, 32, 8, 15, 10, 32768, ("random_graph",), gate=("lds",)),
    # kcap = pow2(3 + 43 * 96) = 8,192 (step 42: 4,096); 8,192 heap entries alone are 64 KiB
    _c("gate-kcap", 128, 32, 3, 43, 10, 32768, ("random_graph",), gate=("kcap", "lds")),
]
BY_NAME = {c.name: c for c in CASES}

# branch of the issue's table -> the cases that reach it
BRANCHES = {
    "1 scalar decode": ("scalar-m24", "scalar-m24-whole", "scalar-dim102", "scalar-dim102-m26"),
    "2 vector decode, cpp 1 / 2 / 4 / 16": ("vec-m4", "vec-m8", "vec-m16", "vec-m64"),
    "3 n = 256": ("n256-random", "n256-windowed"),
    "4 parallel 1 and 8, ns < parallel": ("par1", "vec-m4", "n256-random", "few-starts"),
    "5 empty heap": ("dry-heap", "no-lists"),
    "6 END with nknown < k": ("no-lists",),
    "7 equal distances": ("ties",),
    "8 bucketing overflow": ("scalar-m24", "n256-windowed", "no-lists"),
    "9 in-step duplicates": ("scalar-m24", "scalar-m24-whole", "vec-m4", "vec-m8", "vec-m16", "n256-windowed"),
    "10 re-queried ids": ("scalar-m24", "par1"),
    "11 vertex 0": ("vertex0", "no-lists"),
    "12 the gate": ("gate-par9", "gate-nm", "gate-lds", "gate-kcap"),
    "13 uneven teams": ("uneven-teams",),
}


def vec16(case):
    """DrlArgs::vec16 (drl_team_init): the vector decode's condition."""
    cpp = case.m // 4
    return (case.dim + case.m) % 4 == 0 and case.dim % 4 == 0 and case.m % 4 == 0 and cpp & (cpp - 1) == 0


def gate(case):
    """The limits of drl_plan (pm_devloop.cpp) that the case's call is past, from the shape and the budget
    schedule alone: constants of pm_internal.h, team_round_lds of pm_drl.hip.

    This is a restatement in Python, not drl_plan's own answer: the kernel may hold no counters and the
    library has no probe of the gate, so a gate case can only assert host_dev_steps == 0.  If drl_plan's budget
    rule drifted from the lines below, a gate case could fall back for the budget and not for the limit it
    names without a test noticing; the device cases would notice the opposite drift (host_dev_steps 0)."""
    n, P = case.parallel * case.m, case.m // 2
    qn = n // P
    out = set()
    if case.parallel > 8:
        out.add("parallel")
    if n > 256:
        out.add("n")
    if n * case.m > 8192:
        out.add("nm")
    kcap = 1
    while kcap < case.parallel + case.step * n:
        kcap *= 2
    if kcap > 4096:
        out.add("kcap")
    n4 = (n + 3) & ~3
    if kcap * 8 + ((n * case.m + 3) & ~3) * 4 + 9 * n4 * 4 > 64 * 1024:
        out.add("lds")
    PS = -(-case.n // P)
    maxq0, maxq_last = (int(math.sqrt(x) * math.log(x)) for x in (PS, case.n - (P - 1) * PS))   # MaxQueryNum
    support = maxq0 // 2   # SupportBatchNum (RecordStats: partition 0's MaxQueryNum / QueryPerPartition)
    fbn = qmip = 0
    for _ in range(case.q):
        if qmip + case.step * qn >= min(maxq0, maxq_last) or qmip + (case.step - 1) * qn + 2 >= maxq0:
            out.add("budget")
        fbn += case.step * (n // case.m)
        qmip += case.step * qn
        if fbn + case.step * case.parallel + 10 >= support:
            fbn = qmip = 0
    return frozenset(out)


_inputs, _reference = {}, {}


def inputs(case):
    """(vectors, graph, queries [S, q, dim], [(pir_seed, search_seed)] per session); shared by the cases of one shape."""
    from tests import datagen
    key = (case.dim, case.m, case.n, case.graph, case.lone, case.rows)
    if key not in _inputs:
        graph = getattr(datagen, case.graph[0])(case.n, case.m, *case.graph[1:], seed=31)
        if case.lone:
            graph = datagen.lone_id_lists(graph, case.lone, seed=31)
        if case.rows == TIED:
            v, pool = datagen.tied_vectors(case.n, case.dim, 64, seed=32)
        else:
            v, pool = datagen.sift_like_vectors(case.n, case.dim, seed=32), None
        for a in (v, graph):
            a.setflags(write=False)
        _inputs[key] = (v, graph, pool)
    v, graph, pool = _inputs[key]
    rng = np.random.default_rng([33, case.S, case.q])
    if pool is not None:
        qs = pool[rng.integers(0, len(pool), size=(case.S, case.q))]
    else:
        pick = v[rng.integers(0, case.n, size=(case.S, case.q))]
        qs = np.clip(np.rint(pick + rng.normal(0, 8, pick.shape)), 0, 255)
    return v, graph, qs.astype(np.float32), [(300 + i, 400 + i) for i in range(case.S)]


def probe_ids(case, last_answer, i):
    """One batch of ids for a host-path query after the loop: the session's last answer (fetched through PIR
    during the search, so in the localCache unless a maintenance emptied it), then random ids."""
    ids = np.random.default_rng([34, i]).integers(0, case.n, size=case.parallel * case.m).astype(np.uint64)
    got = last_answer[last_answer >= 0].astype(np.uint64)[:len(ids)]
    ids[:len(got)] = got
    return ids


def oracle_run(oracle, case):
    """Independent oracle sessions of the case, computed once and read-only: per session the answers [q, k],
    counts(), the batch-PIR stats after the loop, the trace, and after the probe its rows, the stats and every
    partition's FinishedQueryNum and client state."""
    if case.name not in _reference:
        v, graph, qs, seeds = inputs(case)
        out = []
        for i, (p, s) in enumerate(seeds):
            o = oracle.Graph(v, graph, pir_seed=p, search_seed=s)
            o.Preprocess()
            ans, _, _ = o.SearchLoop(qs[i], case.k, case.step, case.parallel)
            counts, stats, trace = o.counts(), o.pir().stats(), o.trace()
            rows, _ = o.pir().Query(probe_ids(case, ans[-1], i))
            fqn = [o.pir().sub(j).Config()["FinishedQueryNum"] for j in range(case.m // 2)]
            state = [o.pir().sub(j).export_state() for j in range(case.m // 2)]
            for a in (ans, rows, *[x for st in state for x in st.values()]):
                a.setflags(write=False)
            out.append(dict(answers=ans, counts=counts, stats=stats, trace=trace, probe=rows,
                            probe_stats=o.pir().stats(), fqn=fqn, state=state))
        _reference[case.name] = out
    return _reference[case.name]


def trace_sum(ref):
    """The sessions' trace counters added up (max_new: the largest), with counts()'s "total" and "succ"."""
    keys = ref[0]["trace"].keys()
    out = {k: (max if k == "max_new" else sum)(r["trace"][k] for r in ref) for k in keys}
    out["total"], out["succ"] = (sum(r["counts"][j] for r in ref) for j in (0, 1))
    return out

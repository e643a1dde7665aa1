"""Every branch of the device loop's team round against the oracle.

k_team_round (pm_drl.hip) runs after every step of pm_search_loop_batched's device loop: the results'
post-processing, GetVertexInfo's decode, SearchKNN's update with Go's heap order, the next batch and the
batch-PIR bucketing.  The cases of tests/devloop_cases.py drive its scalar and vector decode at every chunk
count, n = 256 positions, parallel 1 to 8, an empty heap, an answer shorter than k, equal distances, the
bucketing's overflow, in-step duplicates, re-queried ids, vertex 0, teams of unequal size and the gate's limits;
tests/test_devloop_cases.py shows from the oracle's trace counts, without a GPU, that each case reaches its branch.

Each case runs twice on fresh sessions with the same seeds, with pm.set_option("device_loop", 1) and with 0, and
both runs are compared bit for bit (ids, counters, XORs: the tolerance is zero) with independent oracle.Graph
runs: the answers, counts(), the batch-PIR counters, and, after one host-path QueryWithMask per session that
reads the device loop's state back (dummy counters, FinishedQueryNum, the localCache index), its rows, the
counters and every partition's FinishedQueryNum and exported client state.  "host_dev_steps" must be
q * step * teams and "host_dev_queries" S * q where the device loop is meant to serve the call, so a silent
fall-back to the host loop fails; both are 0 for the gate cases and for the host runs.
"""
import numpy as np
import pytest

from tests import devloop_cases as D
from tests.test_gpu_parity import STATE_KEYS

pytestmark = pytest.mark.gpu


def run_mode(case, base, mode, ref):
    import pacmann_amd as pm
    v, graph, qs, seeds = D.inputs(case)
    pm.set_option("device_loop", mode)
    try:
        sess = [base.Session(p, s) for p, s in seeds]
        for x in sess:
            x.Preprocess()
        for x in sess:
            x.ctx.timing_reset()
        ans, _, _, _ = pm.search_loop_batched(sess, qs, case.k, case.step, case.parallel, case.ngroups, 4)
        out = dict(answers=ans,
                   dev_steps=sum(x.ctx.timing_get("host_dev_steps")[0] for x in sess),
                   dev_queries=sum(x.ctx.timing_get("host_dev_queries")[1] for x in sess),
                   counts=[x.counts() for x in sess], stats=[x.PIR.stats() for x in sess])
        # after the loop, one host-path batch query per session
        out["probe"] = [x.PIR.QueryWithMask(D.probe_ids(case, ref[i]["answers"][-1], i)) for i, x in enumerate(sess)]
        out["probe_stats"] = [x.PIR.stats() for x in sess]
        P = case.m // 2
        out["fqn"] = [[x.PIR.SubConfig(p)["FinishedQueryNum"] for p in range(P)] for x in sess]
        out["state"] = [[x.PIR.export_state(p) for p in range(P)] for x in sess]
        return out
    finally:
        pm.set_option("device_loop", -1)


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_team_round_case(oracle, name):
    import pacmann_amd as pm
    case = D.BY_NAME[name]
    ref = D.oracle_run(oracle, case)
    v, graph, qs, seeds = D.inputs(case)
    base = pm.PIRGraphInfo(v, graph, pir_seed=1, search_seed=2, ctx=pm.Context(0))
    base.Preprocess()
    assert base.PIR.Config()["PartitionNum"] == case.m // 2
    teams = len(pm.team_sizes(case.S, case.ngroups))
    for mode in (1, 0):
        got = run_mode(case, base, mode, ref)
        print(name, "device_loop", mode, "host_dev_steps", got["dev_steps"], "host_dev_queries", got["dev_queries"])
        if mode == 1 and not case.gate:
            assert got["dev_steps"] == case.q * case.step * teams, (mode, got["dev_steps"])
            assert got["dev_queries"] == case.S * case.q, (mode, got["dev_queries"])
        else:
            assert got["dev_steps"] == 0 and got["dev_queries"] == 0, (mode, got["dev_steps"], got["dev_queries"])
        for i, r in enumerate(ref):
            assert np.array_equal(got["answers"][i], r["answers"]), (mode, i, got["answers"][i], r["answers"])
            assert got["counts"][i] == r["counts"], (mode, i)
            for when in ("stats", "probe_stats"):
                for key in ("FinishedBatchNum", "QueriesMadeInPartition", "PrepCount"):
                    assert got[when][i][key] == r[when][key], (mode, i, when, key)
            rows, ok = got["probe"][i]
            assert np.array_equal(rows, r["probe"]), (mode, i)
            assert not rows[~ok].any(), (mode, i)
            assert got["fqn"][i] == r["fqn"], (mode, i)
            for p, (a, b) in enumerate(zip(got["state"][i], r["state"])):
                for key in STATE_KEYS:
                    assert np.array_equal(a[key], b[key]), (mode, i, p, key)

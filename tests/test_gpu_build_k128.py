"""pm_build_graph_k128 against the oracle's graph, row for row: m from 43 to 64
(int(1.5 m) + self above the 64-key list) through the 128-key kNN and the
unchanged k_prune / k_prune<false>, and m = 32 against pm_build_graph_wide."""
import numpy as np
import pytest

from tests import knn_k128_ref as K
from tests.knn_ref import prune_trace

pytestmark = pytest.mark.gpu


def build_timed(ctx, v, m):
    import pacmann_amd as pm
    ctx.timing(1)
    try:
        ctx.timing_reset()
        g, t = pm.build_graph_k128(v, m, 1.2, 1, ctx)
        runs = {name: ctx.timing_get(name)[0] for name in
                ("knn_prefilter_k128", "knn_prefilter_k128_w", "knn_prefilter_x3", "knn_prefilter_w")}
    finally:
        ctx.timing(0)
    return g, t, runs


def test_degree_64_more_than_32_accepts(ctx, oracle):
    """n = 300, d = 100, m = 64: K = 96 candidates per vertex, and robustPrune
    accepts more than 32 of them (k_prune's second round of the alpha test)."""
    v = np.random.default_rng(41).standard_normal((300, 100)).astype(np.float32)
    cand = oracle.knn(v, v[:1], 96)[0][0]
    acc, _, _ = prune_trace(oracle, v, 0, cand[cand != 0].astype(np.uint32), 64, 1.2)
    assert len(acc) > 32
    g, t, runs = build_timed(ctx, v, 64)
    assert np.array_equal(g, oracle.build_graph(v, 64, 1.2, 1))
    assert runs["knn_prefilter_k128"] == 1 and sum(runs.values()) == 1
    assert 0 <= t["knn_fallback_rows"] <= len(v)


def test_degree_48_wide_rows(ctx, oracle):
    """n = 300, d = 960, m = 48: K = 72, the wide prefilter and k_prune<false>."""
    v = K.clustered_floats(300, 960, centres=6)
    g, _, runs = build_timed(ctx, v, 48)
    assert np.array_equal(g, oracle.build_graph(v, 48, 1.2, 1))
    assert runs["knn_prefilter_k128_w"] == 1 and sum(runs.values()) == 1


def test_degree_43_integers(ctx, oracle):
    """n = 200, d = 128, m = 43 (K = 64: the first m the 64-key build refuses),
    integers 0..255."""
    import pacmann_amd as pm
    v = np.random.default_rng(43).integers(0, 256, (200, 128)).astype(np.float32)
    with pytest.raises(Exception, match=r"m must be in \[1, 42\]"):
        pm.build_graph_wide(v, 43, 1.2, 1, ctx)
    g, _, _ = build_timed(ctx, v, 43)
    assert np.array_equal(g, oracle.build_graph(v, 43, 1.2, 1))


def test_smallest_n_at_degree_64(ctx, oracle):
    """n = m + 1 = 65: K = 96 is above n, every other vertex is a candidate (a
    list of exactly m, kept as it is); no row is judged."""
    v = np.random.default_rng(44).standard_normal((65, 24)).astype(np.float32)
    g, t, _ = build_timed(ctx, v, 64)
    assert np.array_equal(g, oracle.build_graph(v, 64, 1.2, 1))
    assert t["knn_fallback_rows"] == 0
    assert (g < 65).all() and (g != np.arange(65, dtype=np.uint32)[:, None]).all()


def test_degree_32_equals_the_64_key_build(ctx, oracle):
    """m = 32, d = 100, clustered: the graph is pm_build_graph_wide's (and the
    oracle's) and no more rows reach the brute-force kernel."""
    import pacmann_amd as pm
    v = K.clustered_floats(600, 100)
    g, t, _ = build_timed(ctx, v, 32)
    gw, tw = pm.build_graph_wide(v, 32, 1.2, 1, ctx)
    assert np.array_equal(g, gw) and np.array_equal(g, oracle.build_graph(v, 32, 1.2, 1))
    print(f"BUILD_FALLBACK n=600 d=100 m=32: 128 keys {t['knn_fallback_rows']}, 64 keys {tw['knn_fallback_rows']}")
    assert t["knn_fallback_rows"] <= tw["knn_fallback_rows"]
